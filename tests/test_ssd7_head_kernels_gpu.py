"""The kernels behind `SSD7.fused_blocks(..., heads=True)` against their contracts (include/ssdhip.h, csrc/ssdhip_heads7.hip):
ssdhip_ssd7_pack_heads and ssdhip_ssd7_head_wgrad_nhwc_bf16.  Expected values are tests/np_ssd7_heads.py's float64.  Shapes
(tests/np_ssd7_heads.py: KERNEL_CASES, SPLIT_CASES) are the smallest at which the kernel can still go wrong: maps of 1 x 1, 2 x 2, 4 x 4,
9 x 8 and 5 x 3 at batch 1 and 3 -- all inside one 256-position chunk, where the whole contraction is border handling -- for each of
the three input widths and packed widths of 40, 30 and 48 (no padding rows), plus 3 x 26 x 25 cases whose plan has five splits of two
chunks, the last of one."""
import ctypes
import functools

import numpy as np
import pytest

from tests import np_ssd7_heads as ref

pytestmark = pytest.mark.gpu

CASES = ref.KERNEL_CASES + ref.SPLIT_CASES
ids = lambda cases: ["cin%d-b%d-%dx%d-%d+%d" % c for c in cases]
BADARG = -1


@functools.lru_cache(maxsize=None)
def _case(case, kind):
    """Operands (bf16-representable float64; x [B, H, W, Cin], the packed dy [B, H, W, 48] with values in its padding channels too) and
    the float64 references of one case, computed once and never written to."""
    cin, b, h, w, nc, nl = case
    rng = np.random.RandomState(hash(case) % (2 ** 31))
    if kind == "exact":
        x = rng.randint(-4, 5, size=(b, h, w, cin)).astype(np.float64)
        dy = rng.randint(-4, 5, size=(b, h, w, ref.CP)).astype(np.float64)
    else:
        x, dy = (ref.conv.to_bf16(rng.standard_normal(s)) for s in ((b, h, w, cin), (b, h, w, ref.CP)))
    d = dict(x=x, dy=dy)
    d["dwc"], d["dbc"], d["dwl"], d["dbl"] = ref.param_grads(x, dy, nc, nl)
    d["adwc"], d["adbc"], d["adwl"], d["adbl"] = ref.param_grads(np.abs(x), np.abs(dy), nc, nl)
    for v in d.values():
        v.setflags(write=False)
    return d


def _map(a):
    """float64 NHWC array -> (B, C, H, W) bf16 CUDA tensor with NHWC memory."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16).cuda().permute(0, 3, 1, 2)


def _filters(wt, channels_last=True):
    """[n, 3, 3, Cin] float64 -> (n, Cin, 3, 3) bf16 CUDA tensor in either memory order."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(wt)).to(torch.bfloat16).cuda().permute(0, 3, 1, 2)
    return t if channels_last else t.contiguous()


def _bits(t):
    import torch
    return t.contiguous().view(torch.int16).cpu().numpy()


def _bf16_bits_of(a):
    import torch
    return _bits(torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16))


def _likes(case, dtype, channels_last):
    import torch
    cin, _b, _h, _w, nc, nl = case
    mk = lambda n: torch.empty((n, cin, 3, 3), dtype=dtype, device="cuda")
    return tuple(t.contiguous(memory_format=torch.channels_last) if channels_last else t for t in (mk(nc), mk(nl)))


def _wgrad(case, kind, dtype=None, channels_last=True, x=None, dy=None):
    import torch
    from ssd_keras_amd import _native as nat
    d = _case(case, kind)
    like_c, like_l = _likes(case, dtype or torch.float32, channels_last)
    out = nat.ssd7_head_wgrad(_map(d["x"] if x is None else x), _map(d["dy"] if dy is None else dy), like_c, like_l)
    torch.cuda.synchronize()
    assert out[0].stride() == like_c.stride() and out[2].stride() == like_l.stride() and all(t.dtype == like_c.dtype for t in out)
    return out


def _np(t):
    return t.double().cpu().numpy()


def _want(d):
    """The references in the outputs' (n, Cin, 3, 3) index order."""
    return d["dwc"].transpose(0, 3, 1, 2), d["dbc"], d["dwl"].transpose(0, 3, 1, 2), d["dbl"]


@pytest.mark.parametrize("channels_last", [False, True], ids=["contiguous", "channels_last"])
def test_pack_launch_writes_every_byte(channels_last):
    """Buffers prefilled with 0xFF bytes; ONE launch for four maps (Cin 64, 48, 48, 32; packed widths 40, 30, 48 and 40): the forward image
    equals conv_bn_elu_pack of cat([conf, loc, zero rows]), the flipped one conv_bn_elu_pack of its flip(2, 3).transpose(0, 1), the
    bias [conf | loc | zeros], byte for byte."""
    import torch
    from ssd_keras_amd import _native as nat
    rng = np.random.RandomState(11)
    shapes = [(64, 24, 16), (48, 18, 12), (48, 32, 16), (32, 24, 16)]
    wc = [_filters(rng.standard_normal((nc, 3, 3, cin)), channels_last) for cin, nc, _ in shapes]
    wl = [_filters(rng.standard_normal((nl, 3, 3, cin)), channels_last) for cin, _, nl in shapes]
    assert all(t.is_contiguous() != channels_last for t in wc + wl)
    bc = [torch.from_numpy(rng.standard_normal(nc)).to(torch.bfloat16).cuda() for _, nc, _ in shapes]
    bl = [torch.from_numpy(rng.standard_normal(nl)).to(torch.bfloat16).cuda() for _, _, nl in shapes]
    fwd, flipped, bias = nat.ssd7_head_images(wc, wl)
    for t in fwd + flipped + bias:
        t.view(torch.uint8).fill_(0xFF)
    nat.ssd7_pack_heads(wc, wl, bc, bl, fwd, flipped, bias)
    torch.cuda.synchronize()
    for i, (cin, nc, nl) in enumerate(shapes):
        pad = ref.CP - nc - nl
        cat = torch.cat([wc[i], wl[i]] + ([torch.zeros((pad, cin, 3, 3), dtype=torch.bfloat16, device="cuda")] if pad else []))
        assert np.array_equal(_bits(fwd[i]), _bits(nat.conv_bn_elu_pack(cat).reshape(-1)))
        assert np.array_equal(_bits(flipped[i]), _bits(nat.conv_bn_elu_pack(cat.flip(2, 3).transpose(0, 1)).reshape(-1)))
        want_bias = torch.cat([bc[i], bl[i], torch.zeros((pad,), dtype=torch.bfloat16, device="cuda")])
        assert np.array_equal(_bits(bias[i]), _bits(want_bias))
    # the packed convolution run on those buffers is the two heads' convolutions: forward through the image and the bias
    x = ref.conv.to_bf16(rng.standard_normal((2, 5, 3, 64)))
    y = nat.ssd7_conv_bias(_map(x), fwd[0], bias[0], ref.CP, 3)
    want = ref.forward(x, _np(wc[0].permute(0, 2, 3, 1)), _np(bc[0]), _np(wl[0].permute(0, 2, 3, 1)), _np(bl[0]))
    got = _np(y.permute(0, 2, 3, 1))
    assert np.all(np.abs(got - want) <= 2.0 ** -8 * np.abs(want) + 1e-2) and not got[..., 40:].any()


@pytest.mark.parametrize("case", CASES, ids=ids(CASES))
def test_exact_arithmetic(case):
    """x, dy in -4 .. 4: every partial and total is an integer of at most 16 * 1950 < 2^24, so float32 outputs must equal the exact
    integers bit for bit (both memory orders of the parameters) and bf16 outputs their one rounding.  dy's padding channels carry
    values as well: they belong to no output."""
    import torch
    from ssd_keras_amd import _native as nat
    d = _case(case, "exact")
    assert max(np.abs(d[k]).max() for k in ("adwc", "adwl", "adbc", "adbl")) <= 16 * 1950
    if case in ref.SPLIT_CASES:
        splits, per, chunks, last = nat.ssd7_head_wgrad_plan(case[1], case[2], case[3], case[0])[:4]
        print("plan of %s: %d splits of %d chunks, the last %d (of %d)" % (case, splits, per, last, chunks))
        assert splits > 1 and per > 1 and last < per
    want = _want(d)
    for channels_last in (False, True):
        got = _wgrad(case, "exact", torch.float32, channels_last)
        assert all(np.array_equal(_np(g), w) for g, w in zip(got, want))
        got = _wgrad(case, "exact", torch.bfloat16, channels_last)
        assert all(np.array_equal(_bits(g), _bf16_bits_of(w)) for g, w in zip(got, want))


def _excess(got, want, k_len, mag, rounded):
    """error - bound per element: 2^-8 |want| (the bf16 rounding, where there is one) + K 2^-24 sum |a||b| (a length-K float32 sum): the
    bound of tests/test_ssd7_conv_kernels_gpu.py."""
    return np.abs(got - want) - ((2.0 ** -8 * np.abs(want) if rounded else 0.0) + k_len * 2.0 ** -24 * mag)


@pytest.mark.parametrize("case", CASES, ids=ids(CASES))
def test_random_values(case):
    """N(0, 1) operands rounded to bf16.  K: the positions the kernel adds up, 256 per chunk of the padded list.  float32 output carries
    no rounding term, bf16 output one."""
    import torch
    from ssd_keras_amd import _native as nat
    d = _case(case, "random")
    k_len = nat.ssd7_head_wgrad_plan(case[1], case[2], case[3], case[0])[2] * 256
    want = _want(d)
    mags = (d["adwc"].transpose(0, 3, 1, 2), d["adbc"], d["adwl"].transpose(0, 3, 1, 2), d["adbl"])
    for dtype in (torch.float32, torch.bfloat16):
        got = _wgrad(case, "random", dtype)
        worst = [float(_excess(_np(g), w, k_len, m, dtype == torch.bfloat16).max()) for g, w, m in zip(got, want, mags)]
        print("random %s (%s): largest (error - bound) dw_conf %.3g db_conf %.3g dw_loc %.3g db_loc %.3g" % ((case, dtype) + tuple(worst)))
        assert max(worst) <= 0


@pytest.mark.parametrize("case", [CASES[9], CASES[10], CASES[11], CASES[15]], ids=ids([CASES[9], CASES[10], CASES[11], CASES[15]]))
def test_no_cross_talk(case):
    """A NaN in one channel of dy reaches dw[co], db[co] of the head that owns the channel and nothing else; a NaN in a padding channel
    reaches nothing; a NaN in one input channel of x reaches only dw[..., ci] of both heads.  The 48-channel operands run as two
    32-channel blocks whose last 16 lanes read past the position's values: what those lanes see must stay out of every sum."""
    d = _case(case, "exact")
    cin, b, h, w, nc, nl = case
    want = _want(d)
    for co in (nc // 2, nc + nl - 1, ref.CP - 1):
        dy = d["dy"].copy()
        dy[b - 1, h // 2, w // 2, co] = np.nan
        got = [_np(g) for g in _wgrad(case, "exact", dy=dy)]
        if co >= nc + nl:                                               # a padding channel
            assert all(np.array_equal(g, wt) for g, wt in zip(got, want))
            continue
        hw, hb, row = (0, 1, co) if co < nc else (2, 3, co - nc)
        assert np.isnan(got[hw][row]).all() and np.isnan(got[hb][row])
        for i, (g, wt) in enumerate(zip(got, want)):
            keep = np.ones(g.shape[0], dtype=bool)
            if i in (hw, hb):
                keep[row] = False
            assert np.array_equal(g[keep], wt[keep])
    ci = cin - 1
    x = d["x"].copy()
    x[0, h - 1, 0, ci] = np.nan
    got = [_np(g) for g in _wgrad(case, "exact", x=x)]
    for g, wt in ((got[0], want[0]), (got[2], want[2])):
        assert np.isnan(g[:, ci]).any() and np.array_equal(np.delete(g, ci, axis=1), np.delete(wt, ci, axis=1))
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[3], want[3])


@pytest.mark.parametrize("case", [CASES[3], CASES[15], CASES[16]], ids=ids([CASES[3], CASES[15], CASES[16]]))
def test_two_calls_are_bit_equal(case):
    import torch
    for dtype in (torch.float32, torch.bfloat16):
        a, b = _wgrad(case, "random", dtype), _wgrad(case, "random", dtype)
        assert all(torch.equal(s, t) for s, t in zip(a, b))


def test_refusals_launch_nothing():
    """Misaligned pointers, Cp != 48, a workspace that is too small, an input width the kernel does not have, too many packed rows, a
    negative stride: SSDHIP_E_BADARG, the sentinel-filled outputs and workspace untouched."""
    import torch
    from ssd_keras_amd import _native as nat
    lib = nat.load()
    x = torch.zeros((2, 4, 4, 64), dtype=torch.bfloat16, device="cuda")
    dy = torch.ones((2, 4, 4, 64), dtype=torch.bfloat16, device="cuda")
    outs = [torch.full((n,), 7.0, dtype=torch.float32, device="cuda") for n in (24 * 9 * 64 + 8, 24 + 8, 16 * 9 * 64 + 8, 16 + 8)]
    ws = torch.full((1 << 20,), 7.0, dtype=torch.float32, device="cuda")
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    need = int(lib.ssdhip_ssd7_head_wgrad_workspace_bytes(2, 4, 4, 64, 48))
    assert 0 < need <= ws.numel() * 4

    def call(xp=None, dyp=None, o=None, cin=64, cp=48, nc=24, nl=16, bf16=0, sc=None, sl=None, wsp=None, nbytes=need):
        o = o or [p(t) for t in outs]
        return lib.ssdhip_ssd7_head_wgrad_nhwc_bf16(xp or p(x), dyp or p(dy), o[0], o[1], o[2], o[3], 2, 4, 4, cin, cp, nc, nl, bf16, sc, sl,
                                                    wsp or p(ws), nbytes, stream)

    assert call(xp=p(x, 2)) == BADARG and call(dyp=p(dy, 8)) == BADARG and call(wsp=p(ws, 4)) == BADARG
    for i in range(4):                                                  # float32 outputs on a 2-byte boundary; bf16 ones on an odd address
        o = [p(t) for t in outs]
        o[i] = p(outs[i], 2)
        assert call(o=o) == BADARG
        o[i] = p(outs[i], 1)
        assert call(o=o, bf16=1) == BADARG
        o[i] = None
        assert call(o=o) == BADARG
    assert call(cp=40) == BADARG and call(cp=64) == BADARG
    assert call(nbytes=need - 1) == BADARG and call(nbytes=0) == BADARG
    assert call(cin=40) == BADARG and call(cin=16) == BADARG and call(cin=128) == BADARG
    assert call(nc=40, nl=16) == BADARG and call(nc=0) == BADARG and call(nl=0) == BADARG
    bad = (ctypes.c_longlong * 4)(576, 1, -192, 64)
    assert call(sc=bad) == BADARG and call(sl=bad) == BADARG
    assert lib.ssdhip_ssd7_head_wgrad_workspace_bytes(2, 4, 4, 40, 48) == 0 and lib.ssdhip_ssd7_head_wgrad_workspace_bytes(2, 4, 4, 64, 40) == 0
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in outs + [ws])
    xm, dym = x.permute(0, 3, 1, 2), dy.permute(0, 3, 1, 2)
    like = lambda n, cin=64, dtype=torch.bfloat16: torch.empty((n, cin, 3, 3), dtype=dtype, device="cuda")
    with pytest.raises(nat.SsdHipError):
        nat.ssd7_head_wgrad(xm, dym, like(24), like(16))                # dy is 64 wide, not the packed 48
    with pytest.raises(nat.SsdHipError):
        nat.ssd7_head_wgrad(xm, dym[:, :48].contiguous(memory_format=torch.channels_last), like(40), like(16))
    with pytest.raises(nat.SsdHipError):
        nat.ssd7_head_wgrad(xm, dym[:, :48].contiguous(memory_format=torch.channels_last), like(24), like(16, dtype=torch.float32))
    assert call() == 0                                                  # and the good call is accepted
    torch.cuda.synchronize()
    assert not bool((outs[0][:24 * 9 * 64] == 7.0).any()) and bool((outs[0][24 * 9 * 64:] == 7.0).all())
    assert not bool((outs[2][:16 * 9 * 64] == 7.0).any()) and bool((outs[2][16 * 9 * 64:] == 7.0).all())
    assert bool((outs[1][24:] == 7.0).all()) and bool((outs[3][16:] == 7.0).all())


def test_pack_launch_refusals():
    """ssdhip_ssd7_pack_heads: nine maps, none, a missing buffer, an input width it does not have, 49 packed rows, a negative stride and an
    odd pointer are SSDHIP_E_BADARG; nothing is launched, the buffers stay as they were."""
    import torch
    from ssd_keras_amd import _native as nat
    lib = nat.load()
    wc = torch.zeros((24, 64, 3, 3), dtype=torch.bfloat16, device="cuda")
    wl = torch.zeros((16, 64, 3, 3), dtype=torch.bfloat16, device="cuda")
    bc, bl = torch.zeros((24,), dtype=torch.bfloat16, device="cuda"), torch.zeros((16,), dtype=torch.bfloat16, device="cuda")
    (f,), (t,), (pb,) = nat.ssd7_head_images([wc], [wl])
    for buf in (f, t, pb):
        buf.fill_(7.0)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda tensor, off=0: tensor.data_ptr() + off
    good = dict(conf_w=p(wc), loc_w=p(wl), conf_b=p(bc), loc_b=p(bl), fwd=p(f), flipped=p(t), bias=p(pb), cin=64, nc=24, nl=16,
                strides=list(wc.stride()) + list(wl.stride()))

    def call(n=1, **change):
        a = dict(good, **change)
        ptr = lambda v: (ctypes.c_void_p * max(n, 1))(*[v] * max(n, 1))
        ints = lambda v: (ctypes.c_int * max(n, 1))(*[v] * max(n, 1))
        return lib.ssdhip_ssd7_pack_heads(n, ptr(a["conf_w"]), ptr(a["loc_w"]), ptr(a["conf_b"]), ptr(a["loc_b"]), ptr(a["fwd"]),
                                          ptr(a["flipped"]), ptr(a["bias"]), ints(a["cin"]), ints(a["nc"]), ints(a["nl"]),
                                          (ctypes.c_longlong * (8 * max(n, 1)))(*(a["strides"] * max(n, 1))), stream)

    assert call(n=9) == BADARG and call(n=0) == BADARG
    for name in ("conf_w", "loc_w", "conf_b", "loc_b", "fwd", "flipped", "bias"):
        assert call(**{name: None}) == BADARG and call(**{name: good[name] + 1}) == BADARG
    assert call(cin=40) == BADARG and call(nc=33) == BADARG and call(nl=0) == BADARG
    assert call(strides=good["strides"][:6] + [-1, 1]) == BADARG
    assert lib.ssdhip_ssd7_pack_heads(1, None, None, None, None, None, None, None, None, None, None, None, stream) == BADARG
    torch.cuda.synchronize()
    assert all(bool((buf == 7.0).all()) for buf in (f, t, pb))
    with pytest.raises(nat.SsdHipError):
        nat.ssd7_pack_heads([wc], [wl], [bc], [bl], [t], [f], [pb])     # the two images swapped
    with pytest.raises(nat.SsdHipError):
        nat.ssd7_pack_heads([wc.float()], [wl.float()], [bc], [bl], [f], [t], [pb])
    assert call() == 0 and call(n=8) == 0                               # the good call, and eight maps
