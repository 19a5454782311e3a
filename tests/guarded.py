"""Guard bands around kernel operands and outputs (tests/test_conv_guard_gpu.py; tests/test_conv_guard_cpu.py turns it on itself).
Plain torch, any device.  GPU AddressSanitizer is not available to this suite, so a band of known bytes on either side of a tensor is the
instrument: a store that leaves an output changes a band byte (`bands_intact`), a load that leaves an operand AND reaches a result
changes the result when the band's content changes (run with bands of FILLS and compare bits), a store that is skipped leaves the
payload's prefill (0xFF bytes: NaN in bf16 and float32) in the result.

  banded(values, fill_byte, band_bytes)     -> a view of `values`' dtype and shape whose storage sits `band_bytes` into ONE uint8 buffer
                                               filled with `fill_byte`; the view keeps the buffer (`guard_buffer`, `guard_band`, `guard_bytes`)
  banded_empty(shape, dtype, device, ...)   -> the same without values: the payload filled with `payload_byte`
  bands_intact(t, fill_byte)                -> every byte before and after the payload still equals `fill_byte` (synchronise first)
  guarded_outputs(monkeypatch, module, ...) -> context manager: `module._empty_nhwc` hands out banded, prefilled maps and records them;
                                               `module._nhwc_bf16` / `_filter_nhwc` record the data_ptr of what they return
  band_bytes(dilation, width, cin)          -> the band-size rule
  receptive_mask(...)                       -> the outputs one input pixel reaches, from the tap arithmetic alone

Fill bytes: 0x00 the baseline (what fresh device memory usually holds); 0xFF -- bf16 0xFFFF and float32 0xFFFFFFFF are NaN; 0x7F -- bf16
0x7F7F is the largest finite value (3.39e38): max, ReLU and pooling drop a NaN operand but never a huge finite one."""
import contextlib

import numpy as np

FILLS = (0x00, 0xFF, 0x7F)
POISON = 0xFF                 # an output's prefill: NaN wherever a kernel does not store
MIN_BAND = 1 << 20
ALIGN = 256


def band_bytes(dilation=1, width=0, cin=0):
    """At least 1 MiB and at least 4 * dilation * (W + 2) * Cin * 2 bytes -- four times the largest displacement a kernel adds to a
    buffer descriptor's base: `dilation` rows of W + 2 pixels of Cin bf16 values (fc6: dilation 6, W = 19, Cin = 512) -- rounded up to a
    multiple of 256 so that the payload keeps the alignment of an allocation of its own."""
    need = max(MIN_BAND, 4 * int(dilation) * (int(width) + 2) * int(cin) * 2)
    return -(-need // ALIGN) * ALIGN


def _torch():
    import torch
    return torch


def banded_empty(shape, dtype, device, fill_byte, band, payload_byte=POISON, nhwc=False):
    """An uninitialised-looking tensor of `shape` between two bands: the payload holds `payload_byte`, the bands `fill_byte`.
    nhwc: `shape` is (B, H, W, C), the result its (B, C, H, W) view (the layout of _native's maps and filters)."""
    torch = _torch()
    assert band > 0 and band % ALIGN == 0, band
    shape = tuple(int(n) for n in shape)
    nbytes = int(np.prod(shape, dtype=np.int64)) * torch.empty((), dtype=dtype).element_size()
    buf = torch.full((band + nbytes + band,), int(fill_byte), dtype=torch.uint8, device=device)
    buf[band:band + nbytes] = int(payload_byte)
    t = buf[band:band + nbytes].view(dtype).view(shape)
    if nhwc:
        assert len(shape) == 4
        t = t.permute(0, 3, 1, 2)
    t.guard_buffer, t.guard_band, t.guard_bytes = buf, band, nbytes
    return t


def banded(values, fill_byte, band, nhwc=False):
    """`values` (a tensor; its elements in C order are the payload) copied between two bands of `fill_byte`, on values' device."""
    t = banded_empty(values.shape, values.dtype, values.device, fill_byte, band, 0, nhwc)
    (t.permute(0, 2, 3, 1) if nhwc else t).copy_(values)
    return t


def bands_intact(t, fill_byte):
    buf, band, nbytes = t.guard_buffer, t.guard_band, t.guard_bytes
    return bool((buf[:band] == int(fill_byte)).all()) and bool((buf[band + nbytes:] == int(fill_byte)).all())


class Record:
    """What guarded_outputs saw: `outputs` (every map handed out, in order) and `seen` (data_ptr of every tensor that `_nhwc_bf16` and
    `_filter_nhwc` returned = what the launch reads)."""

    def __init__(self, fill_byte):
        self.fill_byte, self.outputs, self.seen = fill_byte, [], set()

    def intact(self):
        return all(bands_intact(t, self.fill_byte) for t in self.outputs)

    def handed_out(self, t):
        return any(t.data_ptr() == o.data_ptr() and t.shape == o.shape for o in self.outputs)


@contextlib.contextmanager
def guarded_outputs(monkeypatch, module, fill_byte, band, payload_byte=POISON):
    """While it is open `module._empty_nhwc` (ssd_keras_amd._native's one allocator of output maps: conv_chain's `_chain_walk` and
    conv1_block allocate through it too) returns maps whose payload holds `payload_byte` between bands of `fill_byte`."""
    rec = Record(fill_byte)
    real_map, real_filter = module._nhwc_bf16, module._filter_nhwc

    def empty_nhwc(b, h, w, c, dtype, device):
        rec.outputs.append(banded_empty((b, h, w, c), dtype, device, fill_byte, band, payload_byte, nhwc=True))
        return rec.outputs[-1]

    def nhwc_bf16(t, name):
        out = real_map(t, name)
        rec.seen.add(out[0].data_ptr())
        return out

    def filter_nhwc(weight, *args, **kwargs):
        out = real_filter(weight, *args, **kwargs)
        rec.seen.add(out.data_ptr())
        return out

    with monkeypatch.context() as m:
        m.setattr(module, "_empty_nhwc", empty_nhwc)
        m.setattr(module, "_nhwc_bf16", nhwc_bf16)
        m.setattr(module, "_filter_nhwc", filter_nhwc)
        yield rec


def bits(t):
    """A bf16 map's bit patterns (int16, the map's shape): what "bit-identical" compares."""
    torch = _torch()
    assert t.dtype == torch.bfloat16
    return t.view(torch.int16)


def same_bits(a, b):
    return a.shape == b.shape and bool((bits(a) == bits(b)).all())


def _sync(t):
    if t.is_cuda:
        _torch().cuda.synchronize(t.device)


class Operands:
    """One entry's operands, each in a banded buffer of its own: `arg` is what the test's `call(arg, relu)` takes, `maps` the input
    maps ((B, C, H, W) views, the ones the non-finite checks poison), `others` filters, biases, packed filters, and `uncopied` those
    of them that pass through `_nhwc_bf16` / `_filter_nhwc`, whose result must be the banded view itself."""

    def __init__(self, fill_byte, arg, maps, others, uncopied=None):
        self.fill_byte, self.arg, self.maps, self.others = fill_byte, arg, list(maps), [t for t in others if t is not None]
        self.uncopied = list(self.maps + self.others if uncopied is None else uncopied)
        for t in self.maps + self.others:
            assert t.data_ptr() - t.guard_buffer.data_ptr() == t.guard_band and t.guard_band % ALIGN == 0 and t.guard_bytes % 2 == 0


def guarded_call(monkeypatch, module, call, ops, band, what):
    """One call with guarded outputs -> the list of its results.  Checks that the entry took the geometry, that every result is one of
    the prefilled maps, that no operand was copied on its way to the launch, and property B: the bands of every map handed out, and
    of every operand, are intact."""
    with guarded_outputs(monkeypatch, module, ops.fill_byte, band) as rec:
        outs = call(ops.arg)
    assert outs is not None and all(o is not None for o in outs), what + ": geometry must be supported"
    outs = list(outs)
    _sync(outs[0])
    assert outs and all(rec.handed_out(o) for o in outs) and len(rec.outputs) == len(outs), what + ": a result that _empty_nhwc did not allocate"
    for t in ops.uncopied:
        assert t.data_ptr() in rec.seen, what + ": the wrapper copied an operand, the launch does not read the banded one"
    assert rec.intact(), what + ": bytes outside an output were written (band fill 0x%02X)" % ops.fill_byte
    assert all(bands_intact(t, ops.fill_byte) for t in ops.maps + ops.others), what + ": bytes around an operand were written"
    return outs


def check_written_confined_deaf(monkeypatch, module, ops_by_fill, call, wants, band, what):
    """Properties A, B and C of one entry on one case.  ops_by_fill: {fill byte: Operands} with the same payloads; wants: the exact
    result of every map the entry returns, on the operands' device, in the maps' (B, C, H, W) shape.
    A: every result, allocated full of 0xFF, equals its exact value element for element (under the first fill; C carries it to the
    others).  B: guarded_call, under every fill.  C: the results under the band fills are bit-identical.  Returns the first fill's."""
    results = []
    for fill, ops in ops_by_fill.items():
        outs = guarded_call(monkeypatch, module, call, ops, band, what)
        assert len(outs) == len(wants), what
        for i, (o, want) in enumerate(zip(outs, wants) if not results else ()):
            assert o.shape == want.shape, (what, i, o.shape, want.shape)
            wrong = o != want                            # (equality of values: a NaN left of the prefill differs from everything)
            n = int(wrong.sum())
            assert n == 0, "%s: map %d, band fill 0x%02X: %d of %d elements are not the exact result, the first at (b, c, h, w) = %s" % (
                what, i, fill, n, wrong.numel(), tuple(int(v) for v in wrong.nonzero()[0]))
        results.append((fill, outs))
    fill0, first = results[0]
    for fill, outs in results[1:]:
        for i, (a, b) in enumerate(zip(first, outs)):
            assert same_bits(a, b), "%s: map %d differs between band fills 0x%02X and 0x%02X: bytes outside an operand reach the result" % (
                what, i, fill0, fill)
    return first


@contextlib.contextmanager
def poisoned(maps, index):
    """Inside: maps[i][index[i]] = NaN for every i with an index (None: untouched); restored on the way out."""
    saved = [None if ix is None else m[ix].clone() for m, ix in zip(maps, index)]
    try:
        for m, ix in zip(maps, index):
            if ix is not None:
                m[ix] = float("nan")
        yield
    finally:
        for m, ix, s in zip(maps, index, saved):
            if ix is not None:
                m[ix] = s


def edge_images(b):
    """The first image, the last, and a middle one where there is one."""
    return sorted({0, b - 1, b // 2}) if b >= 3 else list(range(b))


def check_image_isolation(monkeypatch, module, ops, call, clean, band, what, out_of_map=None):
    """Property D, images: with every element of ONE image NaN (the same image index in every input map), every other image of
    every result is bit-identical to `clean`.  Needs B >= 2."""
    b = ops.maps[0].shape[0]
    assert b >= 2 and all(m.shape[0] == b for m in ops.maps) and all(c.shape[0] == b for c in clean)
    for bad in edge_images(b):
        with poisoned(ops.maps, [bad] * len(ops.maps)):
            outs = guarded_call(monkeypatch, module, call, ops, band, what)
        keep = [i for i in range(b) if i != bad]
        for i, (o, c) in enumerate(zip(outs, clean)):
            assert same_bits(o[keep], c[keep]), "%s: map %d: a NaN image %d of %d changed another image's output" % (what, i, bad, b)


def check_member_isolation(monkeypatch, module, ops, call, clean, band, what):
    """Property D, grouped launches: with ONE whole member NaN, every other member's result is bit-identical to `clean`."""
    n = len(ops.maps)
    assert n >= 2 and len(clean) == n
    for bad in edge_images(n):
        with poisoned(ops.maps, [slice(None) if i == bad else None for i in range(n)]):
            outs = guarded_call(monkeypatch, module, call, ops, band, what)
        for i in range(n):
            assert i == bad or same_bits(outs[i], clean[i]), "%s: a NaN member %d changed member %d's output" % (what, bad, i)


def edge_pixels(b, h, w, c):
    """(b, h0, w0, c0): the first pixel of the first image, a centre pixel, the last pixel of the last image."""
    return [(0, 0, 0, 0), (b // 2, h // 2, w // 2, c // 2), (b - 1, h - 1, w - 1, c - 1)]


def check_element_locality(monkeypatch, module, ops, call, clean, geometry, band, what, which=0, others_unchanged=False):
    """Property D, elements (one layer, no ReLU, no pool, filters without zeros): with ONE element of the input map ops.maps[0] NaN,
    result `which` is NaN in all channels exactly where receptive_mask says a tap reads that pixel, and every other element of it keeps
    its bits.  others_unchanged: the other results are those of other problems of a grouped launch and keep their bits too (a
    pool_keep entry's pooled map does not: what a pool makes of a NaN in its window is not specified)."""
    torch = _torch()
    k, stride, pad, dil = geometry
    x, = ops.maps
    b, c, h, w = x.shape
    for pos in edge_pixels(b, h, w, c):
        with poisoned([x], [(pos[0], pos[3], pos[1], pos[2])]):
            outs = guarded_call(monkeypatch, module, call, ops, band, what)
        mask = torch.from_numpy(receptive_mask((b, h, w), pos[:3], k, stride, pad, dil)).to(x.device)
        for i, (o, cl) in enumerate(zip(outs, clean)):
            if i != which:
                assert not others_unchanged or same_bits(o, cl), "%s: NaN at %s changed result %d" % (what, pos, i)
                continue
            o, cl = o.permute(0, 2, 3, 1), cl.permute(0, 2, 3, 1)                      # [B, Ho, Wo, C]
            assert o.shape[:3] == mask.shape, (what, o.shape, mask.shape)
            assert bool(torch.isnan(o[mask]).all()), "%s: NaN at %s: an output that reads it is not NaN" % (what, pos)
            assert bool((bits(o)[~mask] == bits(cl)[~mask]).all()), "%s: NaN at %s changed an output that has no tap on it" % (what, pos)


def _reached(n_out, n_in, at, k, stride, pad, dil):
    """[n_out] bool: output o has a tap on input `at` -- o * stride - pad + t * dil == at for some t in 0 .. k - 1."""
    assert 0 <= at < n_in
    return np.array([any(o * stride - pad + t * dil == at for t in range(k)) for o in range(n_out)], dtype=bool)


def receptive_mask(x_shape, pos, k, stride, pad, dil):
    """[B, Ho, Wo] bool: the outputs of a k x k convolution (stride, zero padding, dilation) of a [B, H, W, .] map that read the input
    pixel pos = (b, h0, w0).  From the tap arithmetic alone: no convolution is run."""
    b, h, w = x_shape[:3]
    ho, wo = (h + 2 * pad - dil * (k - 1) - 1) // stride + 1, (w + 2 * pad - dil * (k - 1) - 1) // stride + 1
    assert ho >= 1 and wo >= 1
    mask = np.zeros((b, ho, wo), dtype=bool)
    mask[pos[0]] = np.outer(_reached(ho, h, pos[1], k, stride, pad, dil), _reached(wo, w, pos[2], k, stride, pad, dil))
    return mask
