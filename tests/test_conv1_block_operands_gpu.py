"""Operand assembly of the fused conv1 block (csrc/ssdhip_conv64.hip, FRONT): the producers build conv1_1's B operand from dword
reads of the image patch, shifted by the parity of the halo column.  A wrong shift or run boundary gives a plausible picture with
Gaussian data, so these cases make every one of the 27 taps visible on its own: one-hot first-layer filters copy tap k = kh*9 + kw*3 + ci
into channel k, an identity second layer passes it through, and the expectation is plain indexing of the image on the CPU.
All comparisons are on bit patterns."""
import pytest

SHAPES = [
    (1, 18, 34),    # two tiles across + a border; even and odd halo columns
    (2, 9, 17),     # odd W: the second image row and the second image start at a 2-byte offset (the two-byte path)
    (1, 1, 1),
    (1, 3, 2),
    (1, 16, 24),    # the 8-column tile shape (patch rows of 72 bytes instead of 120)
]


def _image(B, H, W):
    """x[b, h, w, c] = (7 h + 3 w + c + 11 b) % 251 + 1: distinct small integers, exact in bf16 (NHWC, float32)."""
    import torch
    b = torch.arange(B).view(B, 1, 1, 1)
    h = torch.arange(H).view(1, H, 1, 1)
    w = torch.arange(W).view(1, 1, W, 1)
    c = torch.arange(3).view(1, 1, 1, 3)
    return ((7 * h + 3 * w + c + 11 * b) % 251 + 1).float()


def _tap_filters():
    """w1 (64, 3, 3, 3) [cout, ci, kh, kw]: channel k < 27 is one-hot on tap (kh, kw, ci) of k = kh*9 + kw*3 + ci; w2 (64, 64, 3, 3): identity
    on the centre tap (float32)."""
    import torch
    w1 = torch.zeros((64, 3, 3, 3))
    for k in range(27):
        w1[k, k % 3, k // 9, (k % 9) // 3] = 1.0
    w2 = torch.zeros((64, 64, 3, 3))
    for k in range(64):
        w2[k, k, 1, 1] = 1.0
    return w1, w2


def _expected(x):
    """[B, 64, H, W]: channel k at (h, w) is x[b, h + kh - 1, w + kw - 1, ci], 0 outside the image; channels 27 .. 63 are 0.  Indexing only."""
    import torch
    B, H, W, _ = x.shape
    xp = torch.zeros((B, H + 2, W + 2, 3))
    xp[:, 1:H + 1, 1:W + 1] = x
    out = torch.zeros((B, 64, H, W))
    for k in range(27):
        kh, kw, ci = k // 9, (k % 9) // 3, k % 3
        out[:, k] = xp[:, kh:kh + H, kw:kw + W, ci]
    return out


@pytest.mark.parametrize("shape", SHAPES + [(1, 37, 53)])
def test_tap_expectation_is_a_convolution(shape):
    """No GPU: the indexed expectation equals float32 conv2d -> conv2d of the same tensors exactly (every value is a small integer)."""
    import torch
    import torch.nn.functional as F
    x = _image(*shape)
    w1, w2 = _tap_filters()
    want = torch.relu(F.conv2d(torch.relu(F.conv2d(x.permute(0, 3, 1, 2), w1, None, 1, 1)), w2, None, 1, 1))
    assert torch.equal(_expected(x), want)
    assert torch.equal(x.to(torch.bfloat16).float(), x)


def _bits(t):
    import torch
    return t.permute(0, 2, 3, 1).contiguous().view(torch.int16).cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_every_tap_lands_in_its_channel(shape):
    import torch
    from ssd_keras_amd import _native as nat
    x = _image(*shape)
    w1, w2 = _tap_filters()
    dev = lambda t: t.to(torch.bfloat16).cuda()
    zero = torch.zeros((64,), dtype=torch.bfloat16, device="cuda")
    got = nat.conv1_block(dev(x).permute(0, 3, 1, 2), dev(w1.permute(0, 2, 3, 1)).permute(0, 3, 1, 2), zero,
                          dev(w2.permute(0, 2, 3, 1)).permute(0, 3, 1, 2), zero, relu=True, pool=False)
    want = _expected(x).to(torch.bfloat16)
    assert got.shape == want.shape
    bad = (_bits(got) != _bits(want)).nonzero()
    assert bad.numel() == 0, "%d outputs differ; first (b, h, w, channel = kh*9 + kw*3 + ci): %s" % (bad.shape[0], bad[0].tolist())


def _gaussian(shape, seed):
    import torch
    B, H, W = shape
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = (torch.randn((B, H, W, 3), generator=g, device="cuda") * 60).to(torch.bfloat16).permute(0, 3, 1, 2)
    w1 = (torch.randn((64, 3, 3, 3), generator=g, device="cuda") / 5).to(torch.bfloat16).permute(0, 3, 1, 2)
    b1 = torch.randn((64,), generator=g, device="cuda").to(torch.bfloat16)
    w2 = (torch.randn((64, 3, 3, 64), generator=g, device="cuda") / 24).to(torch.bfloat16).permute(0, 3, 1, 2)
    b2 = torch.randn((64,), generator=g, device="cuda").to(torch.bfloat16)
    return x, w1, b1, w2, b2


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_pooled_block_equals_the_two_kernels(shape):
    import torch
    from ssd_keras_amd import _native as nat
    x, w1, b1, w2, b2 = _gaussian(shape, 100 * shape[1] + shape[2])
    base = nat.conv3x3_c64(nat.conv3x3_cin3(x, w1, b1, relu=True), w2, b2, relu=True, pool=True)
    got = nat.conv1_block(x, w1, b1, w2, b2, relu=True, pool=True)
    assert got.shape == base.shape
    assert torch.equal(got.view(torch.int16), base.view(torch.int16))
    for _ in range(2):
        assert torch.equal(nat.conv1_block(x, w1, b1, w2, b2, relu=True, pool=True).view(torch.int16), got.view(torch.int16))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(3, 37, 53), (3, 37, 54), (7, 150, 150)])   # odd width: two-byte path; even widths: dword path
@pytest.mark.parametrize("pool", [True, False])
def test_image_result_does_not_depend_on_the_batch_around_it(pool, shape):
    """An image alone and as image b of a batch: in the batch its tiles sit at other places of the workgroups' tile sequences, so their
    patches travel through the other register set of the double-buffered requests and into the other halo buffer; the output must not
    change.  (A workgroup only walks more than one tile when there are more tiles than compute units: the 700 tiles of the last shape.)"""
    import torch
    from ssd_keras_amd import _native as nat
    x, w1, b1, w2, b2 = _gaussian(shape, 100 * shape[1] + shape[2])
    x = x.permute(0, 2, 3, 1).contiguous()
    batch = _bits(nat.conv1_block(x.permute(0, 3, 1, 2), w1, b1, w2, b2, relu=True, pool=pool))
    for b in range(shape[0]):
        one = nat.conv1_block(x[b:b + 1].contiguous().permute(0, 3, 1, 2), w1, b1, w2, b2, relu=True, pool=pool)
        assert torch.equal(batch[b:b + 1], _bits(one)), "image %d" % b
