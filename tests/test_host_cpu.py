"""CPU-only checks: the C-ABI library loads and exports every symbol include/ssdhip.h declares; host-side
logic of the drop-in surface (argument validation, anchors, containers, model graphs) without a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from ssd_keras_amd import synthetic as syn
from tests import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    """The library build() writes, as `_native.load()` declares it (every export typed from SIGNATURES)."""
    from ssd_keras_amd import _native as nat
    from ssd_keras_amd import build
    assert build.build() == nat.lib_path()
    return nat.load()


def test_library_exports_every_declared_symbol(lib):
    hdr = open(os.path.join(ROOT, "include", "ssdhip.h")).read()
    names = sorted(set(re.findall(r"\b(ssdhip_[a-z_0-9]+)\s*\(", hdr)))
    assert len(names) >= 10
    for n in names:
        assert hasattr(lib, n), n
    assert lib.ssdhip_abi_version() == 1
    assert b"workspace" in lib.ssdhip_strerror(-2)


def _header_prototypes():
    """{name: (return type, [parameter types])} of every prototype in include/ssdhip.h, comments and preprocessor lines stripped."""
    src = open(os.path.join(ROOT, "include", "ssdhip.h")).read()
    src = re.sub(r"/\*.*?\*/|//[^\n]*|^\s*#[^\n]*", " ", src, flags=re.S | re.M)
    protos = {}
    for ret, name, params in re.findall(r"([^;{}]*?)\b(ssdhip_[a-z_0-9]+)\s*\(([^;{}]*)\)\s*;", src):
        assert name not in protos, "declared twice: " + name
        params = [" ".join(p.split()) for p in params.split(",")] if params.strip() not in ("", "void") else []
        # drop each parameter's name: the type is what precedes it
        protos[name] = (" ".join(ret.split()), [p if "*" in p.rsplit(" ", 1)[-1] else p.rsplit(" ", 1)[0] for p in params])
    return protos


def test_signature_table_matches_the_header():
    """_native.SIGNATURES, the ctypes declaration of every export, against the C prototypes: ctypes does not notice a mismatch (a
    `long long` or a `double` declared as c_int is silently truncated or misread), so the table is checked argument by argument."""
    from ssd_keras_amd import _native as nat
    scalar = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "size_t": ctypes.c_size_t, "double": ctypes.c_double,
              "float": ctypes.c_float}

    def matches(ctype, declared):
        if "*" in ctype:
            return declared in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(declared, ctypes._Pointer)
        key = " ".join(w for w in ctype.split() if w != "const")
        assert key in scalar, "no ctypes kind for C type %r" % ctype
        return declared is scalar[key]

    protos = _header_prototypes()
    assert len(protos) >= 10
    assert sorted(nat.SIGNATURES) == sorted(protos)
    for name, (ret, params) in protos.items():
        declared_ret, declared_args = nat.SIGNATURES[name]
        assert matches(ret, declared_ret), "%s returns %s, declared %s" % (name, ret, declared_ret)
        assert len(declared_args) == len(params), "%s takes %d arguments, declared %d" % (name, len(params), len(declared_args))
        for i, (ctype, declared) in enumerate(zip(params, declared_args)):
            assert matches(ctype, declared), "%s argument %d is %s, declared %s" % (name, i, ctype, declared)


def test_integration_doc_names_every_export():
    """VERDICT r4 row b: every entry point of include/ssdhip.h has its row (verbatim name) in INTEGRATION.md."""
    hdr = open(os.path.join(ROOT, "include", "ssdhip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    names = sorted(set(re.findall(r"\b(ssdhip_[a-z_0-9]+)\s*\(", hdr)))
    assert not [n for n in names if n not in doc]


def test_workspace_sizes(lib):
    d = lib.ssdhip_decode_workspace_bytes(32, 8732, 21, 200, 400, 0, 0)
    assert 32 * 8732 * (16 + 20 * 8) <= d < 2 * 32 * 8732 * (16 + 20 * 8)
    d64 = lib.ssdhip_decode_workspace_bytes(32, 8732, 21, 200, 400, 0, 1)              # float64 predictions: its own, larger layout
    assert 32 * 8732 * (40 + 20 * 13) <= d64 < 2 * 32 * 8732 * (40 + 20 * 13)
    assert lib.ssdhip_decode_workspace_bytes(32, 8732, 21, 200, 400, 0, 2) == 0        # unknown element type
    assert lib.ssdhip_decode_workspace_bytes(0, 8732, 21, 200, 400, 0, 0) == 0
    assert lib.ssdhip_encode_workspace_bytes(32, 8732, 21, 256) >= 256 * 4        # one matched anchor per ground truth box: no similarity matrix
    assert lib.ssdhip_loss_workspace_bytes(32, 8732, 21) >= 2 * 32 * 8732 * 4


def test_product_does_not_import_the_oracle():
    pkg = os.path.join(ROOT, "ssd_keras_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                src = open(os.path.join(dirpath, f)).read()
                assert "np_oracle" not in src and "from oracle" not in src and "import oracle" not in src, f


def test_no_gpu_means_loud_failure():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from ssd_keras_amd import _native as nat
    from ssd_keras_amd.ssd_encoder_decoder.ssd_output_decoder import decode_detections
    y = np.zeros((1, 10, 18), np.float32)
    with pytest.raises(Exception):
        decode_detections(y, img_height=10, img_width=10)           # no CPU fallback
    with pytest.raises(nat.SsdHipError):
        nat.require_cuda(torch.zeros(3), "x")


def test_encoder_host_logic_matches_reference_anchors():
    from ssd_keras_amd.ssd_encoder_decoder.ssd_input_encoder import DegenerateBoxError, SSDInputEncoder
    z = util.load("anchors")
    for name, cfg in (("tiny", syn.TINY), ("ssd7", syn.SSD7_300), ("ssd300", syn.SSD300_VOC), ("ssd512", syn.SSD512_COCO)):
        enc = SSDInputEncoder(**cfg)
        assert np.array_equal(np.concatenate([b.reshape(-1, 4) for b in enc.boxes_list]), z[name + "_centroids_clip0"])
        assert enc.n_classes == cfg["n_classes"] + 1
    enc = SSDInputEncoder(**syn.TINY)
    assert len(enc.boxes_list) == 4 and enc.boxes_list[0].shape == (8, 8, 4, 4) and enc.n_boxes == 4
    t = enc.generate_encoding_template(2)
    assert t.shape == (2, 340, 18) and np.all(t[:, :, :6] == 0) and np.array_equal(t[0, :, 6:10], t[0, :, 10:14])
    with pytest.raises(DegenerateBoxError):
        enc._pack_ground_truth([np.array([[1, 5, 5, 5, 9.]])])
    gt, off, mx = enc._pack_ground_truth([np.zeros((0, 5)), np.array([[1, 1, 1, 5, 9.], [2, 0, 0, 3, 3]])])
    assert list(off) == [0, 0, 2] and mx == 2 and gt.shape == (2, 5)
    for bad in (dict(scales=[0.1, 0.2]), dict(variances=[1, 1, 1]), dict(variances=[1, 1, 1, 0]), dict(coords="polar"),
                dict(steps=[1, 2]), dict(offsets=[0.5]), dict(aspect_ratios_per_layer=[[1.0]]),
                dict(min_scale=None, max_scale=None), dict(aspect_ratios_global=[0.0, 1.0])):
        kw = dict(syn.TINY)
        kw.update(bad)
        with pytest.raises(ValueError):
            SSDInputEncoder(**kw)


def test_layers_and_models_on_cpu():
    import torch
    from ssd_keras_amd.keras_layers.keras_layer_AnchorBoxes import AnchorBoxes
    from ssd_keras_amd.keras_layers.keras_layer_DecodeDetections import DecodeDetections
    from ssd_keras_amd.keras_layers.keras_layer_L2Normalization import L2Normalization
    from ssd_keras_amd.models.keras_ssd300 import ssd_300
    from ssd_keras_amd.models.keras_ssd7 import build_model
    from oracle import np_oracle as orc
    ab = AnchorBoxes(300, 300, 0.2, 0.37, aspect_ratios=[1.0, 2.0, 0.5, 3.0, 1.0 / 3.0], this_steps=16, this_offsets=0.5,
                     normalize_coords=True)
    out = ab(torch.zeros(2, 24, 19, 19))
    want = orc.anchor_boxes_layer(2, 300, 300, (19, 19), 0.2, 0.37, [1.0, 2.0, 0.5, 3.0, 1.0 / 3.0], True, 16, 0.5, False,
                                  [0.1, 0.1, 0.2, 0.2], "centroids", True)
    assert out.shape == (2, 19, 19, 6, 8) and np.array_equal(out.numpy(), want)
    assert ab.compute_output_shape((2, 24, 19, 19)) == (2, 19, 19, 6, 8) and ab.get_config()["this_scale"] == 0.2
    l2 = L2Normalization(gamma_init=20, n_channels=8)
    x = torch.randn(2, 8, 5, 5)
    ref = orc.l2_normalization(x.permute(0, 2, 3, 1).numpy(), np.full(8, 20, np.float32))
    np.testing.assert_allclose(l2(x).permute(0, 2, 3, 1).detach().numpy(), ref, rtol=1e-5, atol=1e-6)
    with pytest.raises(ValueError):
        DecodeDetections(normalize_coords=True)
    with pytest.raises(ValueError):
        DecodeDetections(coords="corners", img_height=1, img_width=1)
    m, ps = build_model((300, 300, 3), 5, scales=syn.SSD7_300["scales"], normalize_coords=True, return_predictor_sizes=True)
    assert ps.tolist() == [[37, 37], [18, 18], [9, 9], [4, 4]]
    m.eval()
    with torch.no_grad():
        y = m(torch.zeros(1, 300, 300, 3))
    enc = orc.EncoderOracle(**syn.SSD7_300)
    assert y.shape == (1, 7160, 18)
    assert np.array_equal(y[0, :, -8:].numpy(), enc.generate_encoding_template(1)[0, :, -8:].astype(np.float32))
    np.testing.assert_allclose(y[0, :, :6].sum(-1).numpy(), 1.0, rtol=1e-5)
    m3, ps3 = ssd_300((300, 300, 3), 20, scales=syn.SSD300_VOC["scales"], return_predictor_sizes=True)
    assert ps3.tolist() == [[38, 38], [19, 19], [10, 10], [5, 5], [3, 3], [1, 1]]
    assert sum(p.numel() for p in m3.parameters()) == 26285486
    with pytest.raises(ValueError):
        ssd_300((300, 300, 3), 20, mode="bogus", scales=syn.SSD300_VOC["scales"])
    with pytest.raises(ValueError):
        ssd_300((300, 300, 3), 20)                                   # neither scales nor min/max scale


def test_keras_weight_layout_round_trip():
    """models/keras_weights.py: Keras layer names + HWIO kernels <-> the torch modules (SSD300 and SSD7), by_name semantics."""
    import numpy as np
    import torch
    from ssd_keras_amd.models.keras_ssd300 import ssd_300
    from ssd_keras_amd.models.keras_ssd7 import build_model
    from ssd_keras_amd.models.keras_weights import export_keras_weights, keras_layer_map, load_keras_weights
    torch.manual_seed(0)
    sc = [0.1, 0.2, 0.37, 0.54, 0.71, 0.88, 1.05]
    a = ssd_300((300, 300, 3), 20, mode="training", scales=sc)
    names = set(keras_layer_map(a))
    expect = {"conv1_1", "conv1_2", "conv2_1", "conv2_2", "conv3_1", "conv3_2", "conv3_3", "conv4_1", "conv4_2", "conv4_3", "conv5_1",
              "conv5_2", "conv5_3", "fc6", "fc7", "conv6_1", "conv6_2", "conv7_1", "conv7_2", "conv8_1", "conv8_2", "conv9_1", "conv9_2",
              "conv4_3_norm"} | {s + t for s in ("conv4_3_norm", "fc7", "conv6_2", "conv7_2", "conv8_2", "conv9_2") for t in ("_mbox_conf", "_mbox_loc")}
    assert names == expect                                     # the layer names of models/keras_ssd300.py:274-361
    w = export_keras_weights(a)
    assert w["conv1_1"][0].shape == (3, 3, 3, 64) and w["fc6"][0].shape == (3, 3, 512, 1024) and w["conv4_3_norm"][0].shape == (512,)
    assert w["conv4_3_norm_mbox_conf"][0].shape == (3, 3, 512, 4 * 21)
    # a Keras kernel element [kh, kw, ci, co] is the torch weight [co, ci, kh, kw]
    assert w["conv2_1"][0][1, 2, 5, 7] == a.conv2_1.weight[7, 5, 1, 2].item()
    torch.manual_seed(1)
    b = ssd_300((300, 300, 3), 20, mode="training", scales=sc)
    part = {k: v for k, v in w.items() if not k.startswith("conv9")}          # by_name: missing layers keep their init
    keep = b.conv9_1.weight.clone()
    loaded, missing = load_keras_weights(b, part)
    assert sorted(missing) == ["conv9_1", "conv9_2", "conv9_2_mbox_conf", "conv9_2_mbox_loc"] and torch.equal(b.conv9_1.weight, keep)
    assert torch.equal(a.conv3_2.weight, b.conv3_2.weight) and torch.equal(a.conv4_3_norm.gamma, b.conv4_3_norm.gamma)
    assert torch.equal(a.loc_heads[1].bias, b.loc_heads[1].bias)
    bad = dict(w)
    bad["fc7"] = [w["fc7"][0][:, :, :, :10], w["fc7"][1][:10]]
    with pytest.raises(ValueError):
        load_keras_weights(b, bad)
    # SSD7 incl. BatchNormalization statistics; loaded model computes the same function
    s1 = build_model((64, 64, 3), 3, scales=[0.1, 0.3, 0.5, 0.7, 0.9]).eval()
    for bn in s1.bns:
        bn.running_mean.uniform_(-1, 1)
        bn.running_var.uniform_(0.5, 2)
    s2 = build_model((64, 64, 3), 3, scales=[0.1, 0.3, 0.5, 0.7, 0.9]).eval()
    loaded, missing = load_keras_weights(s2, export_keras_weights(s1), by_name=False)
    assert not missing and "bn3" in loaded and "classes5" in loaded
    x = torch.from_numpy(np.random.RandomState(0).randint(0, 256, size=(2, 64, 64, 3)).astype(np.float32))
    with torch.no_grad():
        assert torch.equal(s1(x), s2(x))


def test_keras_weight_file_loads_end_to_end(tmp_path):
    """`model.load_weights(weights_path, by_name=True)` (ssd300_inference.ipynb:117, ssd300_training.ipynb:162) without h5py: a weight
    FILE in the .npz container (what keras_weights.NPZ_CONVERSION writes next to a Keras .h5) loaded into a fresh SSD300; the loaded
    model computes the same predictions, layer for layer named as in models/keras_ssd300.py."""
    import numpy as np
    import torch
    from ssd_keras_amd.models.keras_ssd300 import ssd_300
    from ssd_keras_amd.models.keras_weights import NPZ_CONVERSION, load_keras_weights, save_keras_weights_npz
    sc = [0.1, 0.2, 0.37, 0.54, 0.71, 0.88, 1.05]
    torch.manual_seed(3)
    a = ssd_300((300, 300, 3), 20, mode="training", scales=sc).eval()
    path = str(tmp_path / "VGG_VOC0712_SSD_300x300.npz")
    save_keras_weights_npz(a, path)
    with np.load(path) as z:
        assert "conv1_1/0" in z.files and "conv1_1/1" in z.files and z["fc6/0"].shape == (3, 3, 512, 1024)       # HWIO, Keras order
    torch.manual_seed(4)
    b = ssd_300((300, 300, 3), 20, mode="training", scales=sc).eval()
    loaded, missing = load_keras_weights(b, path, by_name=True)
    assert not missing and len(loaded) == 36
    for pa, pb in zip(a.parameters(), b.parameters()):
        assert torch.equal(pa, pb)
    x = torch.from_numpy(np.random.RandomState(0).randint(0, 256, size=(1, 300, 300, 3)).astype(np.float32))
    with torch.no_grad():
        assert torch.equal(a(x), b(x))
    compile(NPZ_CONVERSION, "<npz conversion>", "exec")            # the documented one-off conversion script parses
    with pytest.raises(ValueError):
        np.savez(str(tmp_path / "bad.npz"), **{"conv1_1": np.zeros(3)})
        load_keras_weights(b, str(tmp_path / "bad.npz"))


def test_evaluator_ground_truth_packing():
    """The vectorised per-class CSR packing of Evaluator.match_predictions == a per-image loop with the reference's masks."""
    import numpy as np
    from ssd_keras_amd.eval_utils.average_precision_evaluator import Evaluator
    rng = np.random.RandomState(4)
    labels, neutral = [], []
    for i in range(57):
        g = int(rng.randint(0, 6)) if i % 5 else 0
        labels.append(np.stack([rng.randint(1, 5, size=g), rng.randint(0, 50, size=g), rng.randint(0, 50, size=g),
                                rng.randint(50, 99, size=g), rng.randint(50, 99, size=g)], axis=1).astype(np.int64).reshape(-1, 5))
        neutral.append(rng.uniform(size=g) < 0.3)
    labels[3] = []                                                   # an image given as an empty list
    neutral[3] = []
    cat, img, ncat = Evaluator._concat_ground_truth(labels, neutral)
    for c in range(1, 5):
        boxes, off, flags = Evaluator._class_ground_truth(cat, img, ncat, len(labels), c, 0, [1, 2, 3, 4])
        assert off.dtype == np.int32 and off.shape == (58,) and boxes.dtype == np.float64 and flags.dtype == np.uint8
        for i, lab in enumerate(labels):
            lab = np.asarray(lab).reshape(-1, 5)
            m = lab[:, 0] == c
            assert np.array_equal(boxes[off[i]:off[i + 1]], lab[m][:, 1:5].astype(np.float64))
            assert np.array_equal(flags[off[i]:off[i + 1]].astype(bool), np.asarray(neutral[i], dtype=bool).reshape(-1)[m])
    cat, img, ncat = Evaluator._concat_ground_truth(labels, None)
    assert ncat is None and Evaluator._class_ground_truth(cat, img, None, len(labels), 2, 0, [1, 2, 3, 4])[2] is None


def test_entry_points_reject_bad_arguments_before_launching(lib):
    """Argument validation happens on the host, ahead of any launch: callable without a GPU."""
    conv = lib.ssdhip_conv2d_nhwc_bf16
    dummy = ctypes.create_string_buffer(64)
    a = ctypes.addressof(dummy)
    a += (-a) % 16                                                    # a 16-byte aligned, non-null fake pointer (never dereferenced)
    ok_dims = dict(B=1, H=8, W=8, Cin=64, Cout=64, k=3, stride=2, pad=1, dil=1)

    def call(**kw):
        d = dict(ok_dims)
        d.update(kw)
        return conv(a, a, None, a, d["B"], d["H"], d["W"], d["Cin"], d["Cout"], d["k"], d["stride"], d["pad"], d["dil"], 1, None)

    assert conv(None, None, None, None, 1, 8, 8, 64, 64, 3, 2, 1, 1, 1, None) == -1       # SSDHIP_E_BADARG
    for bad in (dict(Cin=48), dict(Cout=32), dict(k=5), dict(stride=0), dict(stride=5), dict(pad=2), dict(pad=-1), dict(dil=0),
                dict(H=2, W=2, pad=0)):
        assert call(**bad) == -1, bad
    same = lib.ssdhip_conv2d_same_nhwc_bf16
    assert same(a, a, None, a, 1, 8, 8, 64, 48, 3, 1, 1, None) == -1
    loss = lib.ssdhip_loss_forward
    assert loss(a, a, 2, 10, 6, 3, 0, 1.0, a, a, a, a, 16, None) == -2                      # SSDHIP_E_WORKSPACE: too small
    assert loss(a, a, 2, 10, 1, 3, 0, 1.0, a, a, a, a, 1 << 20, None) == -1                 # C < 2
    # the largest C the header states (SSDHIP_LOSS_MAX_CLASSES): one more is refused by both directions, the plan and the workspace size
    hdr = open(os.path.join(ROOT, "include", "ssdhip.h")).read()
    cmax = int(re.search(r"#define\s+SSDHIP_LOSS_MAX_CLASSES\s+(\d+)", hdr).group(1))
    back = lib.ssdhip_loss_backward
    plan = (ctypes.c_int * 8)()
    assert cmax >= 250
    assert loss(a, a, 2, 10, cmax + 1, 3, 0, 1.0, a, a, a, a, 1 << 30, None) == -1
    assert back(a, a, a, a, a, 2, 10, cmax + 1, 1.0, a, None) == -1
    assert back(a, a, a, a, a, 2, 10, 1, 1.0, a, None) == -1
    assert lib.ssdhip_loss_plan(a, a, a, a, 2, 10, cmax + 1, plan) == -1 and lib.ssdhip_loss_workspace_bytes(2, 10, cmax + 1) == 0
    assert lib.ssdhip_loss_plan(a, a, a, a, 2, 10, cmax, plan) == 0 and plan[2] == 64 and lib.ssdhip_loss_workspace_bytes(2, 10, cmax) > 0
    assert loss(a, a, 2, 10, cmax, 3, 0, 1.0, a, a, a, a, 16, None) == -2                   # accepted as far as the workspace check


def test_optimizer_steps_refuse_bad_arguments_before_anything_runs(lib):
    """The five optimizer step exports share one host launcher (csrc/ssdhip_optim_step.h) that makes EVERY check before the first
    launch: a refused call returns SSDHIP_E_BADARG (-1) and neither the tick nor an earlier chunk has run.  The addresses are made
    up (16-byte aligned, never dereferenced), so this runs only where no launch can succeed: there an accepted call -- and a check
    that is missing, or that comes after the tick -- ends as SSDHIP_E_LAUNCH (-3).  Three tensors of 0x3fffffff * 4096 values are
    each within the per-tensor limit and together over the grid's."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("made-up device addresses: only where no launch can succeed")
    N, BIG = 3, 0x3fffffff * 4096
    VP, LL = ctypes.c_void_p * N, ctypes.c_longlong * N
    STATE = 1 << 24
    # name: (columns, takes group / state / tick, takes a rule, the last column is the optional vhat)
    exports = {"ssdhip_sgd_momentum_step": (3, False, False, False), "ssdhip_sgd_step": (3, True, True, False),
               "ssdhip_sgd_step_bf16": (4, True, True, False), "ssdhip_adam_step": (5, True, False, True),
               "ssdhip_adam_step_bf16": (6, True, False, True)}

    def columns(ncol):
        return [[(1 << 20) + 4096 * (c * N + k) for k in range(N)] for c in range(ncol)]

    for name, (ncol, has_state, has_rule, has_vhat) in exports.items():
        for tick in ((0, 1) if has_state else (0,)):
            for vhat in ((True, False) if has_vhat else (True,)):

                def call(n=N, cols=None, numel=(8,) * N, group=0, state=STATE, rule=0):
                    cols = columns(ncol) if cols is None else cols
                    if not vhat:
                        cols = cols[:-1] + [None]
                    tail = (group, state) + ((rule, 0) if has_rule else ()) + (tick,) if has_state else (0.1, 0.9, 0.0)
                    return getattr(lib, name)(n, *[c if c is None else VP(*c) for c in cols],
                                              None if numel is None else LL(*numel), *tail, None)

                what = (name, tick, vhat)
                assert call() == -3, what                                        # valid but for the device: it got as far as a launch
                assert call(numel=(BIG,) * N) == -1, what                         # one launch's grid
                assert call(numel=(BIG + 1, 8, 8)) == -1, what                    # one tensor's blocks
                assert call(n=0) == -1 and call(n=-1) == -1 and call(numel=None) == -1, what
                assert call(numel=(8, 0, 8)) == -1 and call(numel=(8, 8, -4)) == -1, what
                for c in range(ncol - (0 if vhat else 1)):
                    for k in range(N):
                        for bad in (4, None):                                     # an address 4 past alignment, a null row
                            cols = columns(ncol)
                            cols[c][k] = None if bad is None else cols[c][k] + bad
                            assert call(cols=cols) == -1, what + (c, k, bad)
                    if not (has_vhat and c == ncol - 1):                          # (a null vhat column is a call without amsgrad)
                        cols = columns(ncol)
                        cols[c] = None
                        assert call(cols=cols) == -1, what + (c,)
                if has_state:
                    assert call(group=64) == -1 and call(group=-1) == -1, what
                    assert call(state=None) == -1 and call(state=STATE + 4) == -1, what
                if has_rule:
                    assert call(rule=2) == -1 and call(rule=-1) == -1, what


def test_autotune_keeps_the_fastest_candidate_and_probes_slow_ones_once(monkeypatch):
    """SSDModel._pick (models/_common.py): best of two bursts per candidate.  MIOpen competes only under SSDHIP_CONV=auto_miopen
    (it goes last and is dropped after one probe call when that alone is slower than three calls of the best so far); by default
    only libssdhip's variants are timed."""
    import time
    import torch
    from ssd_keras_amd.models._common import SSDModel

    class FakeEvent:
        def __init__(self, enable_timing=True):
            self.t = None

        def record(self):
            self.t = time.perf_counter()

        def synchronize(self):
            pass

        def elapsed_time(self, other):
            return (other.t - self.t) * 1e3

    monkeypatch.setattr(torch.cuda, "Event", FakeEvent)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    monkeypatch.setenv("SSDHIP_CONV", "auto_miopen")
    saved = dict(SSDModel._conv_choice)
    SSDModel._conv_choice.clear()
    try:
        calls = {}

        def cand(name, seconds):
            def fn():
                calls[name] = calls.get(name, 0) + 1
                time.sleep(seconds)
            return fn

        m = SSDModel.__new__(SSDModel)
        got = m._pick(("t", 1), {"miopen": cand("miopen", 0.02), "igemm": cand("igemm", 0.002), "igemm6": cand("igemm6", 0.001)})
        assert got == "igemm6" and calls["miopen"] == 2 and calls["igemm"] >= 9 and calls["igemm6"] >= 9
        calls.clear()
        assert m._pick(("t", 2), {"miopen": cand("miopen", 0.001), "igemm": cand("igemm", 0.003)}) == "miopen"
        assert m._pick(("t", 2), {}) == "miopen"                         # cached per key
        monkeypatch.delenv("SSDHIP_CONV", raising=False)                 # default: MIOpen is not probed when the library has a kernel
        calls.clear()
        assert m._pick(("t", 5), {"miopen": cand("miopen", 0.0001), "igemm": cand("igemm", 0.003), "igemm6": cand("igemm6", 0.001)}) == "igemm6"
        assert "miopen" not in calls
        assert m._pick(("t", 6), {"miopen": cand("miopen", 0.0001), "igemm": cand("igemm", 0.003)}) == "igemm" and "miopen" not in calls
        # near-ties ("act" keys): only the two-stage kernel loses one, and then to the FASTEST of the deeper forms within 8 %
        act = lambda i: ("act", (1, 64, 8, 8), 64, 3, 1, True, 1, 1, i)
        assert m._pick(act(0), {"igemm": cand("igemm", 0.0100), "igemm6": cand("igemm6", 0.0105), "halo": cand("halo", 0.0103)}) == "halo"
        assert m._pick(act(1), {"image": cand("image", 0.0100), "halo": cand("halo", 0.0104)}) == "image"      # a deeper form that won stays
        assert m._pick(act(2), {"igemm": cand("igemm", 0.0100), "igemm6": cand("igemm6", 0.0120)}) == "igemm"    # beyond 8 %: no tie
        monkeypatch.setenv("SSDHIP_CONV", "igemm")
        assert m._pick(("t", 3), {"miopen": None, "igemm": None}) == "igemm" and m._pick(("t", 4), {"miopen": None}) == "miopen"
    finally:
        SSDModel._conv_choice.clear()
        SSDModel._conv_choice.update(saved)


def test_all_core_cpu_baseline_helper_runs_and_agrees_with_the_port():
    """bench.py's cpu_baseline.all_cores leg (tools/cpu_decode_all_cores.py in its own process): same detections as the port in
    this process; a bad argument comes back as an error entry instead of an exception."""
    import bench_extra as bx
    from oracle import np_oracle as orc
    enc = orc.EncoderOracle(**syn.TINY)
    y = syn.make_y_pred(enc.generate_encoding_template(1)[0, :, -8:], 3, enc.n_classes, bias=1.0, seed=3)
    kw = dict(confidence_thresh=0.05, iou_threshold=0.45, top_k=50, normalize_coords=True, img_height=96, img_width=128)
    res = bx.cpu_decode_all_cores(y, kw, timeout_s=120)
    assert "error" not in res, res
    want = sum(r.shape[0] for r in orc.decode_detections(y, **kw) if r.size)
    assert res["images"] == 3 and res["detections"] == want and res["value"] > 0 and 1 <= res["cores"] <= 3
    assert "error" in bx.cpu_decode_all_cores(y, dict(kw, no_such_argument=1), timeout_s=120)


def test_fused_sgd_accepts_gradients_that_walk_memory_like_their_parameter():
    """ssd_keras_amd.optimizers.SGD takes a gradient into its one-launch update when it has its parameter's memory order: strides are
    compared only on dimensions with more than one entry -- a 1 x 1 filter is the same memory contiguous or channels_last, and a
    float32 gradient that came with the other stride metadata (csrc/ssdhip_wgrad.hip's 1 x 1 form, round 5) used to fall out of the fused
    launch into the framework's per-tensor arithmetic."""
    import torch
    from ssd_keras_amd.optimizers import SGD
    p = torch.zeros((8, 1, 1, 4)).permute(0, 3, 1, 2)                                     # strides (4, 1, 4, 4): channels_last metadata
    g = torch.zeros((8, 4, 1, 1))                                                         # strides (4, 1, 1, 1)
    assert p.stride() != g.stride() and SGD._same_order(g, p) and SGD._same_order(p, g)
    q = torch.zeros((8, 4, 3, 3)).contiguous(memory_format=torch.channels_last)
    assert SGD._same_order(q.clone(memory_format=torch.preserve_format), q)
    assert not SGD._same_order(torch.zeros((8, 4, 3, 3)), q)                              # a real layout difference
    assert not SGD._same_order(torch.zeros((8, 4, 1, 2)), p)                              # another shape
    b = torch.zeros((7,))
    assert SGD._same_order(b.clone(), b)


def test_step_timeline_tool_finds_steps_by_either_preprocess_kernel(tmp_path):
    """tools/step_timeline.py delimits a bench step by the input-pipeline kernel: `preprocess_kernel` or, since round 5 (four pixels per
    thread), `preprocess3_kernel` -- the tool missed every step of the first trace taken after the rename."""
    import csv
    import json
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import step_timeline
    rows, t = [], 1000
    for step in range(12):
        for name in ("void ssdhip::preprocess3_kernel(float4 const*)", "ssdhip::conv64_kernel<4>(ssdhip::C64Params)",
                     "ssdhip::scan_heads_kernel(ssdhip::HeadParams)", "ssdhip::nms_kernel<2, 512, false>(ssdhip::DecodeParams)"):
            rows.append({"Start_Timestamp": t, "End_Timestamp": t + 500, "Kernel_Name": name, "Queue_Id": 1})
            t += 600
    trace = tmp_path / "trace.csv"
    with open(trace, "w", newline="") as fh:
        w = csv.DictWriter(fh, fieldnames=list(rows[0]))
        w.writeheader()
        w.writerows(rows)
    out = tmp_path / "out.json"
    step_timeline.main(str(trace), str(out))
    got = json.load(open(out))
    assert got["launches"] == 4 and "headline_eager" in got and "headline_timed" in got


def test_encoder_pickles_without_its_device_state():
    """after the first `encode_to_device` the encoder held pinned tensors and HIP events in its __dict__ and could no longer
    be pickled or deep-copied (DataLoader workers, copied generator configs).  The per-process device state stays out of the copy."""
    import copy
    import pickle
    from ssd_keras_amd import synthetic as syn
    from ssd_keras_amd.ssd_encoder_decoder.ssd_input_encoder import SSDInputEncoder

    class Unpicklable:
        def __reduce__(self):
            raise TypeError("a HIP event does not pickle")

    enc = SSDInputEncoder(**syn.TINY)
    enc.__dict__['_pinned_ring'] = {'cuda:0': {'slots': [[None, Unpicklable()]], 'next': 0}}      # what _upload leaves behind
    enc._dev['cuda:0'] = (Unpicklable(), Unpicklable())
    for twin in (pickle.loads(pickle.dumps(enc)), copy.deepcopy(enc)):
        assert '_pinned_ring' not in twin.__dict__ and twin._dev == {}
        assert twin.n_anchors == enc.n_anchors and np.array_equal(twin._anchors_host, enc._anchors_host)
        assert all(np.array_equal(a, b) for a, b in zip(twin.boxes_list, enc.boxes_list))
    assert '_pinned_ring' in enc.__dict__ and len(enc._dev) == 1                                    # the original keeps its state


def test_training_assembly_gate_is_the_kernels_lds_formula():
    """The model gates its one-launch training assembly on libssdhip's own LDS need (a host-side query, no launch): 4- and 6-box maps
    with the packed strides the model builds (multiples of 128 channels), every class count SSD300 / SSD512 are built with."""
    from ssd_keras_amd import _native as nat
    pad = lambda nb, c: -(-(nb * (c + 4)) // 128) * 128
    for c in (2, 6, 21, 35, 36, 40, 41, 81, 91):
        assert nat.assemble_backward_supported(c, [4, 6, 6, 6, 4, 4], [pad(nb, c) for nb in (4, 6, 6, 6, 4, 4)]), c
    assert not nat.assemble_backward_supported(250, [4, 6], [pad(4, 250), pad(6, 250)])       # beyond a CU's LDS: refused, not launched
    assert not nat.assemble_backward_supported(21, [4], [100])                                # a stride the kernel refuses (not % 8)
    assert not nat.assemble_backward_supported(21, [4], [96])                                 # ... or too narrow for 4 x 25 values


def test_slab_kernel_tiling_plan_is_host_arithmetic(monkeypatch):
    """ssdhip_conv3x3_halo_plan (no launch): the pooled slab entries tile the STACKED batch when that takes fewer tiles than tiling every
    image -- SSD300's conv3_3 + pool3 at batch 32: 760 position tiles (x 2 channel tiles = 1 520 units = six rounds of 256 CUs) instead
    of 800 (a seventh round) -- and only then; the magic reciprocal the kernel divides rows with is exact on every row it can ask about."""
    from ssd_keras_amd import _native as nat
    monkeypatch.delenv("SSDHIP_CONVH_STACK", raising=False)
    monkeypatch.delenv("SSDHIP_CONVH_GRID", raising=False)
    assert nat.conv3x3_halo_plan(32, 75, 75, True) == (4, 760, 76, 152)
    assert nat.conv3x3_halo_plan(32, 150, 150, True) == (5, 3040, 0, 19)            # a tie stays on tiles per image
    assert nat.conv3x3_halo_plan(32, 75, 75, False) == (0, 722, 0, 0)               # unpooled, <= 94 wide: the padded position grid
    assert nat.conv3x3_halo_plan(32, 150, 150, False) == (5, 3040, 0, 19)           # unpooled 2-D tiles are never stacked
    assert nat.conv3x3_halo_plan(6, 20, 20, True) == (5, 17, 22, 17)                # even map: two rows of zeros between images
    # un-pooled maps up to 94 wide: the position grid unless 2-D tiles take fewer rounds of 256 workgroups
    assert nat.conv3x3_halo_plan(32, 38, 38, False, 512) == (0, 191, 0, 0)          # SSD300 conv4_x: 764 units, three rounds either way... the grid
    assert nat.conv3x3_halo_plan(32, 75, 75, False, 256) == (0, 722, 0, 0)          # SSD300 conv3_x
    assert nat.conv3x3_halo_plan(16, 64, 64, False, 512) == (4, 256, 0, 4)          # SSD512 conv4_x: 1 024 units = four rounds (grid: 1 060 = five)
    assert nat.conv3x3_halo_plan(16, 32, 32, False, 512) == (4, 64, 0, 2)           # SSD512 conv5_x: 256 units = one round (grid: 276 = two)
    assert nat.conv3x3_halo_plan(2, 64, 64, False, 512)[0] == 0                     # a small batch: one round either way
    assert nat.conv3x3_halo_plan(5, 2, 2, True)[2] == 0                             # a gap narrower than a tile's rows + 2: per image
    for b in range(1, 40):
        for h in (1, 2, 7, 16, 17, 18, 19, 37, 38, 75, 150, 300, 301):
            for w in (1, 5, 16, 31, 32, 33, 75, 150):
                geom, tiles, pitch, rows = nat.conv3x3_halo_plan(b, h, w, True)
                tr, tc = 256 >> geom, 1 << geom
                wt = -(-w // tc)
                per_image = min(b * -(-h // (256 >> g)) * -(-w // (1 << g)) for g in (4, 5))
                if pitch:
                    assert pitch % 2 == 0 and pitch in (h + 1, h + 2) and pitch >= tr + 2
                    assert rows == -(-b * pitch // tr) and tiles == rows * wt and tiles < per_image
                    magic = (1 << 32) // pitch + 1
                    for r in (0, 1, pitch - 1, pitch, b * pitch - 1, b * pitch, (rows + 1) * tr):
                        assert (r * magic) >> 32 == r // pitch
                else:
                    assert tiles == per_image
    monkeypatch.setenv("SSDHIP_CONVH_GRID", "1")
    assert nat.conv3x3_halo_plan(16, 64, 64, False, 512) == (0, 265, 0, 0)
    monkeypatch.setenv("SSDHIP_CONVH_STACK", "0")
    assert nat.conv3x3_halo_plan(32, 75, 75, True) == (4, 800, 0, 5)
    with pytest.raises(nat.SsdHipError):
        nat.conv3x3_halo_plan(0, 75, 75, True)


def test_keras_h5_weight_files_without_h5py(tmp_path):
    """SURVEY 8f row 2 / VERDICT r5 item 9: a Keras `.h5` weight file read WITHOUT an HDF5 library (models/hdf5_lite.py: superblock 0,
    symbol-table groups under version-1 B-trees, local heaps, version-1 object headers with fixed-string attributes, contiguous
    datasets -- what h5py's default libver writes for `model.save_weights`).  This test is the SELF-CONSISTENCY half (the real HDF5
    library's files and the library reading the writer's: tests/test_h5_real_library_cpu.py): (a) the writer's bytes carry the structures of the published format at their documented offsets; (b) an SSD300's
    weighted layers go file -> fresh model bit for bit, with the library-default node size (several symbol table nodes, a B-tree
    over them) and through `model.save()`'s `model_weights` sub-group; (c) reader paths the writer does not produce: big-endian data,
    a version-3 attribute message, 80 links under a two-level B-tree, a continuation block."""
    import struct
    import torch
    from ssd_keras_amd import synthetic as syn
    from ssd_keras_amd.models import hdf5_lite as h5
    from ssd_keras_amd.models.keras_ssd300 import ssd_300
    from ssd_keras_amd.models.keras_weights import export_keras_weights, load_keras_weights, save_keras_weights_h5
    cfg = syn.SSD300_VOC
    mk = lambda seed: (torch.manual_seed(seed), ssd_300((300, 300, 3), cfg["n_classes"], mode="training", scales=cfg["scales"],
                                                       aspect_ratios_per_layer=cfg["aspect_ratios_per_layer"], steps=cfg["steps"],
                                                       offsets=cfg["offsets"]))[1]
    a = mk(1)
    path = str(tmp_path / "weights.h5")
    save_keras_weights_h5(a, path)
    raw = open(path, "rb").read()
    # (a) the published layout: signature, superblock version 0, 8-byte offsets / lengths, end-of-file address, the root entry's header
    assert raw[:8] == b"\x89HDF\r\n\x1a\n" and raw[8] == 0 and raw[13] == 8 and raw[14] == 8
    assert struct.unpack_from("<Q", raw, 40)[0] == len(raw)
    root_header = struct.unpack_from("<Q", raw, 64)[0]
    assert raw[root_header] == 1                                                  # a version-1 object header
    btree, heap = struct.unpack_from("<QQ", raw, 80)
    assert raw[btree:btree + 4] == b"TREE" and raw[heap:heap + 4] == b"HEAP"
    f = h5.File(path)
    names = [n.decode() for n in f.attrs["layer_names"]]
    assert len(names) == len(export_keras_weights(a)) >= 35 and "conv4_3_norm" in names and f.attrs["backend"].item() == b"tensorflow"
    assert [w.decode() for w in f["conv1_1"].attrs["weight_names"]] == ["conv1_1/kernel:0", "conv1_1/bias:0"]
    k = f["conv1_1/conv1_1/kernel:0"]
    assert k.shape == (3, 3, 3, 64) and k.dtype == np.dtype("<f4")                # HWIO, as Keras stores a Conv2D kernel
    # (b) file -> fresh model
    want = export_keras_weights(a)
    for variant in ("plain", "library_k", "model_save"):
        p2 = str(tmp_path / (variant + ".h5"))
        if variant == "plain":
            p2 = path
        elif variant == "library_k":
            root = {"attrs": {"layer_names": np.array([n.encode() for n in want])},
                    "groups": {n: {"attrs": {"weight_names": np.array([("%s/w%d" % (n, i)).encode() for i in range(len(arrs))])},
                                   "groups": {n: {"datasets": {"w%d" % i: arr for i, arr in enumerate(arrs)}}}} for n, arrs in want.items()}}
            h5.write(p2, root, leaf_k=4)                                          # ~36 links: five symbol table nodes under one B-tree node
        else:
            inner = {"attrs": {"layer_names": np.array([n.encode() for n in want])},
                     "groups": {n: {"attrs": {"weight_names": np.array([("%s/w%d" % (n, i)).encode() for i in range(len(arrs))])},
                                    "groups": {n: {"datasets": {"w%d" % i: arr for i, arr in enumerate(arrs)}}}} for n, arrs in want.items()}}
            h5.write(p2, {"groups": {"model_weights": inner, "optimizer_weights": {}}, "attrs": {"keras_version": np.bytes_(b"2.2.4")}})
        b = mk(2)
        loaded, missing = load_keras_weights(b, p2)
        assert sorted(loaded) == sorted(want) and missing == []
        got = export_keras_weights(b)
        assert all(np.array_equal(x, y) for n in want for x, y in zip(got[n], want[n])), variant
    # (c) 80 links with K = 1: forty symbol table nodes, two level-0 B-tree nodes, one level-1 node
    many = {"datasets": {"d%03d" % i: np.full((2,), i, np.int16) for i in range(80)}}
    p3 = str(tmp_path / "many.h5")
    h5.write(p3, many, leaf_k=1)
    f3 = h5.File(p3)
    assert f3.keys() == ["d%03d" % i for i in range(80)] and all(int(f3["d%03d" % i].read()[1]) == i for i in (0, 1, 39, 40, 79))
    top = struct.unpack_from("<Q", open(p3, "rb").read(), 80)[0]
    assert open(p3, "rb").read()[top + 5] == 1                                     # the root's B-tree node is a level-1 node
    # big-endian float data + datatype; a version-3 attribute; a continuation block -- patched / assembled by hand
    p4 = str(tmp_path / "be.h5")
    h5.write(p4, {"datasets": {"x": np.array([1.5, -2.25, 3.0], np.float32)}})
    buf = bytearray(open(p4, "rb").read())
    pos = bytes(buf).find(np.array([1.5, -2.25, 3.0], "<f4").tobytes())
    buf[pos:pos + 12] = np.array([1.5, -2.25, 3.0], ">f4").tobytes()
    dt = bytes(buf).find(bytes([0x11, 0x20, 31, 0, 4, 0, 0, 0]))
    buf[dt + 1] |= 1                                                               # byte order bit: big-endian
    assert np.array_equal(h5.File(bytes(buf))["x"].read(), np.array([1.5, -2.25, 3.0], np.float32))
    # an object header whose attribute sits in a continuation block, the attribute in version 3 (no padding, a character-set byte)
    dt_msg, ds_msg = h5._dtype_message(np.dtype("<i4")), h5._dataspace_message((2,))
    att3 = struct.pack("<BBHHHB", 3, 0, 2, len(dt_msg), len(ds_msg), 0) + b"n\x00" + dt_msg + ds_msg + np.array([7, -9], "<i4").tobytes()
    cont_block = h5._message(0x000C, att3)
    base = bytearray(open(p4, "rb").read())
    cont_addr = len(base)
    base += cont_block
    # the root header: rewrite it behind everything with a continuation message added
    root_header = struct.unpack_from("<Q", base, 64)[0]
    n_msgs, size = struct.unpack_from("<H", base, root_header + 2)[0], struct.unpack_from("<I", base, root_header + 8)[0]
    msgs = bytes(base[root_header + 16:root_header + 16 + size]) + h5._message(0x0010, struct.pack("<QQ", cont_addr, len(cont_block)))
    new_header = struct.pack("<BxHII4x", 1, n_msgs + 2, 1, len(msgs)) + msgs
    struct.pack_into("<Q", base, 64, len(base))
    base += new_header
    struct.pack_into("<Q", base, 40, len(base))
    f5 = h5.File(bytes(base))
    assert np.array_equal(f5.attrs["n"], [7, -9]) and f5.keys() == ["x"]
    # errors are specific
    with pytest.raises(h5.HDF5FormatError, match="not an HDF5 file"):
        h5.File(b"PK\x03\x04" + b"\x00" * 64)
    v2 = bytearray(open(p4, "rb").read())
    v2[8] = 2
    with pytest.raises(h5.HDF5FormatError, match="superblock version 2"):
        h5.File(bytes(v2))
