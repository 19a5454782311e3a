"""tests/guarded.py without a GPU: the receptive-field mask against tests/np_conv_forward.py on a NaN-poisoned input, the harness
against deliberately wrong "kernels" (plain torch functions on CPU tensors that reach memory through the tensor's storage, as a kernel
does through its pointer), and the layout of the banded buffers for every case of tests/forward_exact_cases.py."""
import types

import numpy as np
import pytest
import torch

from tests import forward_exact_cases as cases
from tests import guarded
from tests import np_conv_forward as ref


# ---- the mask -----------------------------------------------------------------------------------------------------------------------
MASK_GEOMETRIES = [  # (B, H, W), k, stride, pad, dilation: geometries of the case tables
    ((2, 19, 19), 3, 2, 1, 1),            # conv6_2: stride 2 behind padding 1, odd map
    ((3, 10, 10), 3, 2, 1, 1),            # ... even map: the last row is never tap 0
    ((3, 5, 5), 3, 1, 0, 1),              # 'valid'
    ((2, 3, 3), 3, 1, 0, 1),              # 'valid', one output pixel
    ((1, 19, 19), 3, 1, 6, 6),            # fc6: dilation 6
    ((1, 13, 13), 3, 1, 0, 2),            # 'valid' with dilation 2
    ((1, 20, 20), 3, 2, 2, 2),            # dilation 2, stride 2
    ((3, 11, 7), 3, 3, 0, 1),             # stride 3 'valid': pixels no output reads
    ((2, 9, 9), 1, 2, 0, 1),              # 1 x 1 stride 2
    ((3, 5, 5), 1, 1, 0, 1),              # 1 x 1
    ((1, 1, 1), 3, 1, 1, 1),              # a single pixel
    ((4, 3, 3), 3, 1, 2, 2),              # a map smaller than the dilated reach
]


@pytest.mark.parametrize("shape,k,s,p,d", MASK_GEOMETRIES)
def test_receptive_mask_is_where_the_reference_convolution_turns_nan(shape, k, s, p, d):
    b, h, w = shape
    rng = np.random.RandomState(7)
    wts = rng.choice(np.array([-1.0, 1.0]), size=(4, k, k, 2))
    empty = 0
    for pos in guarded.edge_pixels(b, h, w, 2):
        x = rng.choice(np.array([-1.0, 1.0]), size=(b, h, w, 2))
        x[pos] = np.nan
        nan = np.isnan(ref.conv_forward(x, wts, None, s, p, d))
        mask = guarded.receptive_mask(shape, pos[:3], k, s, p, d)
        assert nan.shape[:3] == mask.shape and np.array_equal(nan, np.broadcast_to(mask[..., None], nan.shape)), pos
        empty += not mask.any()
    assert empty < 3, "the positions must reach outputs"


# ---- fake kernels -------------------------------------------------------------------------------------------------------------------
def _module():
    """What guarded_outputs patches, with the signatures of ssd_keras_amd._native."""
    m = types.SimpleNamespace()
    m._empty_nhwc = lambda b, h, w, c, dtype, device: torch.empty((b, h, w, c), dtype=dtype, device=device).permute(0, 3, 1, 2)
    m._nhwc_bf16 = lambda t, name: (t, tuple(t.permute(0, 2, 3, 1).shape))
    m._filter_nhwc = lambda weight, ok=True, message=None: weight
    return m


def _raw(t):
    """The whole allocation behind t as a flat tensor of t's dtype, and t's first element's index in it: what a pointer gives a kernel."""
    return torch.empty(0, dtype=t.dtype).set_(t.untyped_storage()), t.storage_offset()


def _pointwise(m, x, w, bias, relu, defect=None):
    """A 1 x 1 convolution + bias [+ ReLU] through the module's helpers, with one deliberate defect."""
    x, (b, h, wd, cin) = m._nhwc_bf16(x, "x")
    wt = m._filter_nhwc(w)
    cout = wt.shape[0]
    y = m._empty_nhwc(b, h, wd, cout, torch.bfloat16, x.device)
    acc = x.permute(0, 2, 3, 1).float() @ wt.reshape(cout, cin).float().T + bias.float()
    if defect in ("band times zero", "max with band"):     # the elements next to x, as a lane one step outside reads them
        xraw, x0 = _raw(x)
        before, after = xraw[x0 - 1].float(), xraw[x0 + x.numel()].float()
    if defect == "band times zero":                        # a border "zeroed" by multiplication
        acc[0, 0, 0, 0] += before * 0.0
        acc[-1, -1, -1, -1] += after * 0.0
    if defect == "neighbour times zero":                   # the same across an image boundary, inside the tensor
        acc[1:, 0, 0, :] += x.permute(0, 2, 3, 1)[:-1, 0, 0, :1].float() * 0.0
    if relu:
        acc = torch.fmax(acc, torch.zeros(()))             # (the hardware's max: a NaN operand is dropped)
    if defect == "max with band":
        assert relu
        acc[0, 0, 0, 0] = torch.fmax(acc[0, 0, 0, 0], before)
    flat = y.permute(0, 2, 3, 1).reshape(-1)
    assert flat.data_ptr() == y.data_ptr()
    val = acc.to(torch.bfloat16).reshape(-1)
    if defect == "unwritten":
        flat[:-1] = val[:-1]
    else:
        flat.copy_(val)
    yraw, y0 = _raw(y)
    if defect == "store before":
        yraw[y0 - 1] = 1.0
    if defect == "store after":
        yraw[y0 + y.numel()] = 1.0
    return y


SHAPE, COUT, BAND = (3, 4, 5, 8), 16, guarded.band_bytes(1, 5, 8)


def _setup(fills=guarded.FILLS):
    rng = np.random.RandomState(3)
    x, w, bias = cases.signs(rng, SHAPE), cases.signs(rng, (COUT, 1, 1, SHAPE[3])), cases.ints(rng, (COUT,), -3, 3)
    pre = ref.conv_forward(x, w, bias, 1, 0, 1)
    to = lambda a: torch.from_numpy(a).to(torch.bfloat16)
    ops = {}
    for fill in fills:
        xb, wb, bb = guarded.banded(to(x), fill, BAND, nhwc=True), guarded.banded(to(w), fill, BAND, nhwc=True), guarded.banded(to(bias), fill, BAND)
        ops[fill] = guarded.Operands(fill, (xb, wb, bb), [xb], [wb, bb], [xb, wb])
    wants = {relu: [to(ref.to_bf16(cases.epilogue(pre, relu))).permute(0, 3, 1, 2)] for relu in (False, True)}
    return ops, wants


def _abc(monkeypatch, defect, relu, fills=guarded.FILLS):
    m = _module()
    ops, wants = _setup(fills)
    return guarded.check_written_confined_deaf(monkeypatch, m, ops, lambda a: [_pointwise(m, *a, relu, defect)], wants[relu], BAND, str(defect))


@pytest.mark.parametrize("relu", [False, True])
def test_a_correct_kernel_passes_all_four(relu, monkeypatch):
    m = _module()
    ops, wants = _setup()
    call = lambda a: [_pointwise(m, *a, relu)]
    clean = guarded.check_written_confined_deaf(monkeypatch, m, ops, call, wants[relu], BAND, "correct")
    guarded.check_image_isolation(monkeypatch, m, ops[0x00], call, clean, BAND, "correct")
    if not relu:
        guarded.check_element_locality(monkeypatch, m, ops[0x00], call, clean, (1, 1, 0, 1), BAND, "correct")
    assert m._empty_nhwc(1, 1, 1, 8, torch.bfloat16, "cpu").untyped_storage().nbytes() == 16, "the patch must be undone"


def test_an_unwritten_element_fails_a(monkeypatch):
    with pytest.raises(AssertionError, match="1 of 960 elements are not the exact result"):
        _abc(monkeypatch, "unwritten", False)


@pytest.mark.parametrize("defect", ["store before", "store after"])
def test_a_store_outside_the_payload_fails_b(defect, monkeypatch):
    for fill in guarded.FILLS:                               # (1.0 = 0x3F80: neither byte is a fill byte)
        with pytest.raises(AssertionError, match="bytes outside an output were written"):
            _abc(monkeypatch, defect, False, (fill,))


def test_a_band_element_times_zero_fails_c_under_nan(monkeypatch):
    _abc(monkeypatch, "band times zero", False, (0x00, 0x7F))
    with pytest.raises(AssertionError, match="differs between band fills 0x00 and 0xFF"):
        _abc(monkeypatch, "band times zero", False, (0x00, 0xFF))
    with pytest.raises(AssertionError, match="differs between band fills 0x00 and 0xFF"):
        _abc(monkeypatch, "band times zero", False)


def test_a_max_with_a_band_element_fails_c_under_the_largest_finite_value_only(monkeypatch):
    _abc(monkeypatch, "max with band", True, (0x00, 0xFF))
    with pytest.raises(AssertionError, match="differs between band fills 0x00 and 0x7F"):
        _abc(monkeypatch, "max with band", True)


def test_a_neighbouring_image_times_zero_fails_d(monkeypatch):
    m = _module()
    ops, wants = _setup()
    call = lambda a: [_pointwise(m, *a, False, "neighbour times zero")]
    clean = guarded.check_written_confined_deaf(monkeypatch, m, ops, call, wants[False], BAND, "finite data cannot tell")
    with pytest.raises(AssertionError, match="changed another image's output"):
        guarded.check_image_isolation(monkeypatch, m, ops[0x00], call, clean, BAND, "neighbour")
    with pytest.raises(AssertionError, match="changed an output that has no tap on it"):
        guarded.check_element_locality(monkeypatch, m, ops[0x00], call, clean, (1, 1, 0, 1), BAND, "neighbour")


def test_a_copied_operand_is_reported(monkeypatch):
    m = _module()
    m._nhwc_bf16 = lambda t, name: (t.clone(memory_format=torch.preserve_format), tuple(t.permute(0, 2, 3, 1).shape))
    ops, wants = _setup()
    with pytest.raises(AssertionError, match="copied an operand"):
        guarded.check_written_confined_deaf(monkeypatch, m, ops, lambda a: [_pointwise(m, *a, False)], wants[False], BAND, "copy")


# ---- layout -------------------------------------------------------------------------------------------------------------------------
def _table_geometries():
    """(dilation, W, channels) of every case the GPU test runs: the arguments of its band_bytes calls."""
    out = [(c[6], c[2], c[3]) for c in cases.SAME_CASES + cases.POOL_CASES]
    out += [(c[8], c[2], c[3]) for c, _ in cases.GENERAL_CASES] + [(c[8], c[2], c[3]) for c in cases.IMAGE_CASES]
    out += [(1, c[2], 64) for c in cases.CIN3_CASES + cases.C64_CASES + cases.BLOCK_CASES]
    out += [(1, c[2], c[3]) for c in cases.GROUP_SHAPES + cases.SLAB_GROUP_SHAPES + [cases.GROUP_1X1] + cases.SLAB_STRIDED_CASES]
    out += [(1, c[2], c[3]) for c, _ in cases.SLAB_CASES + cases.SLAB_POOL_CASES]
    out += [(1, c[2], max([c[3]] + [l[3] for l in c[4]])) for c in cases.CHAIN_CASES]
    return out


def test_band_size_rule_for_every_table_case():
    assert (6, 19, 512) in _table_geometries()               # fc6: the largest displacement a kernel adds to its descriptor base
    for d, w, c in _table_geometries():
        band = guarded.band_bytes(d, w, c)
        assert band % 256 == 0 and band >= 1 << 20 and band >= 4 * d * (w + 2) * c * 2, (d, w, c)
    assert guarded.band_bytes(16, 300, 1024) == 4 * 16 * 302 * 1024 * 2      # past the floor the rule itself decides


@pytest.mark.parametrize("fill", guarded.FILLS)
def test_layout_of_a_banded_map(fill):
    values = torch.arange(2 * 3 * 5 * 8, dtype=torch.float32).reshape(2, 3, 5, 8).to(torch.bfloat16)
    t = guarded.banded(values, fill, BAND, nhwc=True)
    buf = t.guard_buffer
    assert t.shape == (2, 8, 3, 5) and t.dtype == torch.bfloat16 and t.permute(0, 2, 3, 1).is_contiguous()
    assert torch.equal(t.permute(0, 2, 3, 1), values)
    assert buf.dtype == torch.uint8 and buf.numel() == 2 * BAND + values.numel() * 2
    assert t.data_ptr() - buf.data_ptr() == BAND == t.guard_band and BAND % 256 == 0 and t.guard_bytes == values.numel() * 2 and t.guard_bytes % 2 == 0
    assert bool((buf[:BAND] == fill).all()) and bool((buf[BAND + t.guard_bytes:] == fill).all()) and guarded.bands_intact(t, fill)
    for at in (0, BAND - 1, BAND + t.guard_bytes, buf.numel() - 1):          # every band byte counts, the first and the last too
        old = int(buf[at])
        buf[at] = old ^ 0x01
        assert not guarded.bands_intact(t, fill)
        buf[at] = old
    assert guarded.bands_intact(t, fill)
    e = guarded.banded_empty((1, 2, 2, 8), torch.bfloat16, "cpu", fill, BAND, nhwc=True)
    assert bool(torch.isnan(e).all()) and e.shape == (1, 8, 2, 2), "an output's prefill is NaN"
    f = guarded.banded_empty((4,), torch.float32, "cpu", fill, BAND)
    assert bool(torch.isnan(f).all()) and f.guard_bytes == 16
