"""Every kernel path, tile size, box count, tie and threshold of csrc/ssdhip_encode.hip against `orc.EncoderOracle`, on the case table
of tests/encode_cases.py (tests/test_encode_cases_cpu.py proves what each case reaches; tests/golden/encoder_edges.npz pins the oracle
on the edge cases with the reference).  Needs an MI355X.

Bars.  Match map, class columns and anchor / variance columns: exactly the oracle's.  float64 offsets: rtol 1e-12 / atol 1e-13
(device log vs NumPy log); float32: rtol 1e-6 / atol 1e-7.  Two more that need no measured number: the float32-only output --
finalize_kernel<float>, what every training step runs -- is bit-identical to float32(y64) of a float64 call on the same inputs (both
kernels cast the same double), and for 'corners' and 'minmax' on the dyadic configuration, where no log is involved, the float64
output is the oracle's bit for bit.

Where a test owns the output buffers (the C ABI), they lie between 1 MiB bands of each of guarded.FILLS and are prefilled: after one
synchronise the bands are intact and no element still holds its prefill."""
import ctypes

import numpy as np
import pytest

from tests import encode_cases as ec
from tests import guarded

pytestmark = pytest.mark.gpu

BAND = guarded.MIN_BAND
COMBOS = [(c, b) for c in ec.COORDS for b in ec.BORDERS]
F32, F64, BOTH, MATCHES = (True, False, False), (False, True, False), (True, True, True), (False, False, True)
OUTPUTS = (F32, F64, BOTH, MATCHES)
MM_PREFILL = 0x7F                       # an int32 of 0xFF bytes is -1, "background": the match map is prefilled with 0x7F7F7F7F instead


def _torch():
    import torch
    return torch


def encoder(case, **over):
    from ssd_keras_amd.ssd_encoder_decoder.ssd_input_encoder import SSDInputEncoder
    return SSDInputEncoder(**case.config(**over))


def _np(t):
    return None if t is None else t.cpu().numpy()


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.dtype.itemsize in (4, 8)
    kind = np.int32 if a.dtype.itemsize == 4 else np.int64
    return a.shape == b.shape and np.array_equal(a.view(kind), b.view(kind))


def check(kw, want, want_mm, y32=None, y64=None, mm=None, what=""):
    """The bars of the module docstring on whichever outputs are given (NumPy)."""
    what = "%s: " % (what,)
    C = want.shape[2] - 12
    assert not np.isnan(want).any(), what + "the case table has no NaN targets"
    exact = kw["coords"] != "centroids"
    if mm is not None:
        assert mm.dtype == np.int32 and np.array_equal(mm, want_mm), what + "match map differs"
    if y64 is not None:
        assert y64.dtype == np.float64 and y64.shape == want.shape, what
        assert np.array_equal(y64[:, :, :C], want[:, :, :C]), what + "class vectors differ"
        assert np.array_equal(y64[:, :, -8:], want[:, :, -8:]), what + "anchor/variance columns differ"
        np.testing.assert_allclose(y64[:, :, C:C + 4], want[:, :, C:C + 4], rtol=1e-12, atol=1e-13, err_msg=what)
        if exact:
            assert _same_bits(y64, want), what + "float64 output is not the oracle's bit for bit"
    if y32 is not None:
        w32 = want.astype(np.float32)
        assert y32.dtype == np.float32 and y32.shape == want.shape, what
        assert np.array_equal(y32[:, :, :C], w32[:, :, :C]), what + "float32 class vectors differ"
        assert np.array_equal(y32[:, :, -8:], w32[:, :, -8:]), what + "float32 anchor/variance columns differ"
        np.testing.assert_allclose(y32, w32, rtol=1e-6, atol=1e-7, err_msg=what)
        if exact:
            assert _same_bits(y32, w32), what + "float32 output is not float32(oracle) bit for bit"


def run_outputs(enc, gt):
    """{output combination: (y32, y64, mm) as NumPy} of four `encode_to_device` calls; checks that exactly what was asked for comes back
    and that the calls agree bit for bit: the float32-only result (finalize_kernel<float>) with float32 of the float64 one."""
    out = {}
    for o in OUTPUTS:
        r = enc.encode_to_device(gt, want_f32=o[0], want_f64=o[1], want_matches=o[2])
        assert [t is not None for t in r] == list(o), o
        out[o] = tuple(_np(t) for t in r)
    y64 = out[F64][1]
    assert _same_bits(out[F32][0], y64.astype(np.float32)), "float32-only output differs from float32(y64)"
    assert _same_bits(out[BOTH][0], y64.astype(np.float32)) and _same_bits(out[BOTH][1], y64), "the both-outputs call differs"
    assert np.array_equal(out[MATCHES][2], out[BOTH][2]), "the matches-only call differs"
    return out


@pytest.mark.parametrize("coords,border", COMBOS)
def test_output_combinations_on_every_named_case(coords, border):
    for matching in ec.MATCHING:
        for case in ec.NAMED:
            over = dict(coords=coords, border_pixels=border, matching_type=matching)
            want, want_mm = case.oracle(**over)
            out = run_outputs(encoder(case, **over), case.gt)
            check(case.config(**over), want, want_mm, out[F32][0], out[F64][1], out[BOTH][2], what=(case, matching))


# ----------------------------------------------------------------------------------------------------------------------------
# through the C ABI, into buffers the test owns
# ----------------------------------------------------------------------------------------------------------------------------
def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _view_at(shape, dtype, fill, shift, payload=guarded.POISON):
    """(buffer, view): `view` has `shape` and starts `shift` elements into the payload of a banded buffer four elements longer."""
    n = int(np.prod(shape))
    full = guarded.banded_empty((n + 4,), dtype, "cuda", fill, BAND, payload)
    return full, full[shift:shift + n].view(tuple(shape))


def _confined(full, fill, shift, n, payload=guarded.POISON):
    """The bands and the payload elements around the view still hold what they were filled with."""
    torch = _torch()
    slack = torch.cat([full[:shift], full[shift + n:]]).view(torch.uint8)
    return guarded.bands_intact(full, fill) and bool((slack == payload).all())


def abi_args(enc, gt, y32=None, y64=None, mm=None, max_gt=None):
    """(argument dict in the order of ssdhip_encode's parameters without the stream, tensors to keep alive)."""
    torch = _torch()
    from ssd_keras_amd import _native as nat
    lib = nat.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    rows, off, max_g = enc._pack_ground_truth(gt)
    anchors, variances = enc._device_constants(dev)
    gt_d = torch.from_numpy(rows if rows.shape[0] else np.zeros((1, 5))).to(dev)
    off_d = torch.from_numpy(off).to(dev)
    B, N, C, G = len(gt), enc.n_anchors, enc.n_classes, int(rows.shape[0])
    need = lib.ssdhip_encode_workspace_bytes(B, N, C, G)
    assert need > 0
    ws = nat.workspaces.get(dev, 'encode', need)
    args = dict(anchors=_p(anchors), variances=_p(variances), gt=_p(gt_d), gt_offsets=_p(off_d), G_total=G,
                max_gt=int(max_g if max_gt is None else max_gt), B=B, N=N, C=C, img_height=float(enc.img_height),
                img_width=float(enc.img_width), matching_type=1 if enc.matching_type == 'multi' else 0,
                pos_iou_threshold=float(enc.pos_iou_threshold), neg_iou_limit=float(enc.neg_iou_limit), coords=nat.COORDS[enc.coords],
                normalize_coords=int(bool(enc.normalize_coords)), border_pixels=nat.BORDER[enc.border_pixels],
                background_id=int(enc.background_id), y32=_p(y32), y64=_p(y64), mm=_p(mm), ws=_p(ws), ws_bytes=ws.numel())
    return args, (gt_d, off_d, ws, anchors, variances), need


def abi_encode(enc, gt, y32=None, y64=None, mm=None, max_gt=None):
    torch = _torch()
    from ssd_keras_amd import _native as nat
    args, keep, _ = abi_args(enc, gt, y32, y64, mm, max_gt)
    nat.launch('ssdhip_encode', torch.device("cuda", torch.cuda.current_device()), *args.values())
    torch.cuda.synchronize()
    del keep


@pytest.mark.parametrize("case", ec.CLASSES + ec.CLASSES_ODD_N, ids=repr)
def test_store_paths_into_banded_buffers(case):
    """B = 3, N = 336 (the last tile of every image is partial) and N = 329 (odd: with an odd L the images and tiles of one launch start
    on different 16-byte phases), L in {17, 18, 33, 53, 93}: every tile size of both element sizes.  float32-only output at the four
    phases of its first element -- finalize_kernel<float>'s scalar head, float4 body and scalar tail -- then float64, both at once
    with the float32 output off phase, and matches-only."""
    torch = _torch()
    enc = encoder(case)
    kw = case.config()
    want, want_mm = case.oracle()
    B, N, L = want.shape
    assert B == 3 and L in (17, 18, 33, 53, 93) and N in (ec.N_ANCHORS, ec.N_ANCHORS_ODD)
    n = B * N * L
    y64_ref = None
    for fill in guarded.FILLS:
        for shift in (0, 1):
            full, y64 = _view_at((B, N, L), torch.float64, fill, shift)
            abi_encode(enc, case.gt, y64=y64)
            assert _confined(full, fill, shift, n), (case, fill, shift, "float64: bytes outside the output were written")
            got = _np(y64)
            assert not np.isnan(got).any(), (case, fill, shift, "float64: an element was not written")
            check(kw, want, want_mm, y64=got, what=(case, fill, shift))
            y64_ref = got if y64_ref is None else y64_ref
            assert _same_bits(got, y64_ref)
        for shift in (0, 1, 2, 3):
            full, y32 = _view_at((B, N, L), torch.float32, fill, shift)
            assert y32.data_ptr() % 16 == 4 * shift
            abi_encode(enc, case.gt, y32=y32)
            assert _confined(full, fill, shift, n), (case, fill, shift, "float32: bytes outside the output were written")
            got = _np(y32)
            assert not np.isnan(got).any(), (case, fill, shift, "float32: an element was not written")
            check(kw, want, want_mm, y32=got, what=(case, fill, shift))
            assert _same_bits(got, y64_ref.astype(np.float32)), (case, fill, shift, "float32-only output differs from float32(y64)")
        # both outputs (finalize_kernel<double>'s cast loop), the float32 one off phase; and the match map with them
        full32, y32 = _view_at((B, N, L), torch.float32, fill, 3)
        full64, y64 = _view_at((B, N, L), torch.float64, fill, 0)
        fullmm, mm = _view_at((B, N), torch.int32, fill, 1, MM_PREFILL)
        abi_encode(enc, case.gt, y32=y32, y64=y64, mm=mm)
        assert _confined(full32, fill, 3, n) and _confined(full64, fill, 0, n) and _confined(fullmm, fill, 1, B * N, MM_PREFILL), (case, fill)
        assert _same_bits(_np(y64), y64_ref) and _same_bits(_np(y32), y64_ref.astype(np.float32)) and np.array_equal(_np(mm), want_mm)
        # matches only: finalize_kernel<float> without a float32 destination
        fullmm, mm = _view_at((B, N), torch.int32, fill, 2, MM_PREFILL)
        abi_encode(enc, case.gt, mm=mm)
        assert _confined(fullmm, fill, 2, B * N, MM_PREFILL), (case, fill, "match map: bytes outside the output were written")
        got = _np(mm)
        assert not (got == 0x7F7F7F7F).any() and np.array_equal(got, want_mm), (case, fill)


# ----------------------------------------------------------------------------------------------------------------------------
# box counts
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", ec.LADDER)
def test_box_count_ladder(count):
    """1 .. 1024 boxes in one image of three: the 64-row lane loop of the rounds (> 64), the 256- and 1024-thread load loops (> 256),
    match_kernel's LDS on either side of 48 KiB (G48 - 1, G48), the documented limit."""
    case = ec.ladder(count)
    for matching in ec.MATCHING:
        want, want_mm = case.oracle(matching_type=matching)
        enc = encoder(case, matching_type=matching)
        only32 = _np(enc.encode_to_device(case.gt)[0])
        y32, y64, mm = (_np(t) for t in enc.encode_to_device(case.gt, want_f32=True, want_f64=True, want_matches=True))
        check(case.config(matching_type=matching), want, want_mm, only32, y64, mm, what=(case, matching))
        assert _same_bits(only32, y64.astype(np.float32)) and _same_bits(y32, only32), (case, matching)


def test_more_than_1024_boxes_are_refused():
    enc = encoder(ec.ladder(1))
    with pytest.raises(ValueError):
        enc.encode_to_device([ec.EMPTY, ec.random_boxes(ec.ENC_MAX_GT + 1, 5, 3)])


def test_workspace_reuse_between_calls_of_different_size():
    """1024 boxes, then three, then the 1024 again on one stream: the second call finds the large workspace full of the first call's
    partial maxima and matches."""
    big, small = ec.ladder(ec.ENC_MAX_GT), ec.THRESHOLDS[0]
    assert small.gt[0].shape[0] == 3
    enc_big, enc_small = encoder(big), encoder(small)
    first = [_np(t) for t in enc_big.encode_to_device(big.gt, want_f32=True, want_f64=True, want_matches=True)]
    middle = [_np(t) for t in enc_small.encode_to_device(small.gt, want_f32=True, want_f64=True, want_matches=True)]
    third = [_np(t) for t in enc_big.encode_to_device(big.gt, want_f32=True, want_f64=True, want_matches=True)]
    check(small.config(), *small.oracle(), *middle, what=small)
    assert _same_bits(first[0], third[0]) and _same_bits(first[1], third[1]) and np.array_equal(first[2], third[2])
    check(big.config(), *big.oracle(), *first, what=big)


# ----------------------------------------------------------------------------------------------------------------------------
# encode_packed's bound, the empty batch
# ----------------------------------------------------------------------------------------------------------------------------
def test_encode_packed_bound_loose_and_too_small():
    torch = _torch()
    case = ec.CLASSES[0]
    counts = [g.shape[0] for g in case.gt]
    assert counts == [4, 0, 13]
    enc = encoder(case)
    rows, off, max_g = enc._pack_ground_truth(case.gt)
    gt_d, off_d = torch.from_numpy(rows).cuda(), torch.from_numpy(off).cuda()
    G = rows.shape[0]
    want, want_mm = case.oracle()
    exact = [_np(t) for t in enc.encode_packed(gt_d, off_d, G, max_g, 3, True, True, True)]
    check(case.config(), want, want_mm, *exact, what="exact bound")
    # loose: any upper bound gives the same bits (only the LDS tables grow)
    loose = [_np(t) for t in enc.encode_packed(gt_d, off_d, G, G, 3, True, True, True)]
    only32 = _np(enc.encode_packed(gt_d, off_d, G, G, 3)[0])
    assert _same_bits(loose[0], exact[0]) and _same_bits(loose[1], exact[1]) and np.array_equal(loose[2], exact[2])
    assert _same_bits(only32, exact[0])
    # too small: the kernels take g = min(count, bound) boxes of an image -- its FIRST `bound` boxes -- and leave the others alone
    for bound in (4, 1):
        cut = ec.Case("cut_%d" % bound, [g[:bound] for g in case.gt], "the first %d boxes of every image" % bound, **case.over)
        want_cut, want_cut_mm = cut.oracle()
        small = [_np(t) for t in enc.encode_packed(gt_d, off_d, G, bound, 3, True, True, True)]
        check(cut.config(), want_cut, want_cut_mm, *small, what=cut)
        unchanged = [b for b in range(3) if counts[b] <= bound]
        assert 1 in unchanged and _same_bits(small[1][unchanged], exact[1][unchanged]) and np.array_equal(small[2][unchanged], exact[2][unchanged])
        assert _same_bits(_np(enc.encode_packed(gt_d, off_d, G, bound, 3)[0]), small[1].astype(np.float32))
        for fill in guarded.FILLS:                                     # the same through the C ABI: nothing outside the outputs
            full32, y32 = _view_at(want.shape, torch.float32, fill, 1)
            full64, y64 = _view_at(want.shape, torch.float64, fill, 0)
            fullmm, mm = _view_at(want_mm.shape, torch.int32, fill, 0, MM_PREFILL)
            abi_encode(enc, case.gt, y32, y64, mm, max_gt=bound)
            assert _confined(full32, fill, 1, want.size) and _confined(full64, fill, 0, want.size) and _confined(fullmm, fill, 0, want_mm.size, MM_PREFILL)
            assert _same_bits(_np(y64), small[1]) and _same_bits(_np(y32), small[0]) and np.array_equal(_np(mm), small[2])


@pytest.mark.parametrize("coords", ec.COORDS)
def test_batch_without_any_box(coords):
    """G_total == 0: only finalize_kernel runs.  The output is the template with the background column 1, offsets 0, match map -1."""
    case = ec.ALL_EMPTY
    for matching in ec.MATCHING:
        over = dict(coords=coords, matching_type=matching)
        enc = encoder(case, **over)
        out = run_outputs(enc, case.gt)
        want = enc.generate_encoding_template(3)
        C = enc.n_classes
        want[:, :, enc.background_id] = 1
        want[:, :, C:C + 4] = 0
        assert _same_bits(want, case.oracle(**over)[0])
        assert _same_bits(out[F64][1], want) and _same_bits(out[F32][0], want.astype(np.float32)), (coords, matching)
        assert np.array_equal(out[MATCHES][2], np.full((3, ec.N_ANCHORS), -1, np.int32))
        for shift in (0, 3):                                            # and into a banded buffer
            full, y32 = _view_at(want.shape, _torch().float32, 0x7F, shift)
            abi_encode(enc, case.gt, y32=y32)
            assert _confined(full, 0x7F, shift, want.size) and _same_bits(_np(y32), want.astype(np.float32)), (coords, matching, shift)


# ----------------------------------------------------------------------------------------------------------------------------
# argument checks
# ----------------------------------------------------------------------------------------------------------------------------
def test_refused_arguments_touch_nothing():
    """Every SSDHIP_E_BADARG (-1) and SSDHIP_E_WORKSPACE (-2) condition of ssdhip_encode: the return code, and banded, prefilled outputs
    that nobody wrote.  The same arguments with nothing changed are accepted and give the oracle's result."""
    torch = _torch()
    from ssd_keras_amd import _native as nat
    lib = nat.load()
    case = ec.CLASSES[0]
    enc = encoder(case)
    want, want_mm = case.oracle()
    fill = 0x00
    full32, y32 = _view_at(want.shape, torch.float32, fill, 1)
    full64, y64 = _view_at(want.shape, torch.float64, fill, 0)
    fullmm, mm = _view_at(want_mm.shape, torch.int32, fill, 0, MM_PREFILL)
    args, keep, need = abi_args(enc, case.gt, y32, y64, mm)
    stream = nat.current_stream_ptr(torch.device("cuda", torch.cuda.current_device()))
    G, C = args["G_total"], args["C"]
    assert G == 17 and args["max_gt"] == 13

    def rc(**changed):
        assert set(changed) <= set(args)
        return lib.ssdhip_encode(*dict(args, **changed).values(), stream)

    badarg = [dict(anchors=None), dict(variances=None), dict(gt_offsets=None), dict(gt=None), dict(B=0), dict(B=-1), dict(N=0), dict(N=-336),
              dict(C=0), dict(G_total=-1), dict(y32=None, y64=None, mm=None), dict(coords=-1), dict(coords=3), dict(border_pixels=-1),
              dict(border_pixels=3), dict(matching_type=2), dict(matching_type=-1), dict(background_id=-1), dict(background_id=C),
              dict(max_gt=-1), dict(max_gt=G + 1), dict(max_gt=ec.ENC_MAX_GT + 1, G_total=2 * ec.ENC_MAX_GT)]
    for changed in badarg:
        assert rc(**changed) == -1, changed
    for changed in (dict(ws=None), dict(ws_bytes=0), dict(ws_bytes=need - 1)):
        assert rc(**changed) == -2, changed
    assert rc(G_total=0, max_gt=0, gt=None, ws=None) == -2                 # a batch without boxes needs no gt, but still a workspace
    torch.cuda.synchronize()
    for full, shift, n, payload in ((full32, 1, want.size, guarded.POISON), (full64, 0, want.size, guarded.POISON),
                                    (fullmm, 0, want_mm.size, MM_PREFILL)):
        assert _confined(full, fill, shift, n, payload)
        assert bool((full[shift:shift + n].view(torch.uint8) == payload).all()), "a refused call wrote an output"
    assert rc() == 0
    torch.cuda.synchronize()
    check(case.config(), want, want_mm, _np(y32), _np(y64), _np(mm), what="accepted")
    assert _confined(full32, fill, 1, want.size) and _confined(full64, fill, 0, want.size) and _confined(fullmm, fill, 0, want_mm.size, MM_PREFILL)
    del keep


def test_rows_too_long_for_the_lds_are_refused():
    """The one SSDHIP_E_BADARG that comes after the matching kernels: 1024 boxes and C = 121 (L = 133) with a float64 output need
    (64 * 133 + 4) * 8 + 1024 * 84 bytes > 150 KiB in finalize_kernel.  Refused, no output written; float32-only still fits."""
    torch = _torch()
    from ssd_keras_amd import _native as nat
    lib = nat.load()
    big = ec.ladder(ec.ENC_MAX_GT)
    C = 121
    assert (64 * (C + 12) + 4) * 8 + ec.ENC_MAX_GT * (ec.GTBOX_BYTES + 4) > 150 * 1024 > (64 * (C + 12) + 4) * 4 + ec.ENC_MAX_GT * (ec.GTBOX_BYTES + 4)
    case = ec.Case("wide_rows", big.gt, "L = 133", n_classes=C - 1, **big.over)
    enc = encoder(case)
    shape = (3, ec.N_ANCHORS, C + 12)
    n = int(np.prod(shape))
    full64, y64 = _view_at(shape, torch.float64, 0xFF, 0)
    args, keep, _ = abi_args(enc, case.gt, None, y64, None)
    stream = nat.current_stream_ptr(torch.device("cuda", torch.cuda.current_device()))
    assert lib.ssdhip_encode(*args.values(), stream) == -1
    torch.cuda.synchronize()
    assert _confined(full64, 0xFF, 0, n) and bool(torch.isnan(y64).all())
    want, want_mm = case.oracle()
    check(case.config(), want, want_mm, y32=_np(enc.encode_to_device(case.gt)[0]), what=case)
    del keep
