"""Which calls the convolution launch entries of libssdhip accept and which they refuse (tests/test_conv_entry_cpu.py).

Every entry validates its arguments on the host before it launches anything.  Where no launch can succeed (no GPU) an accepted call
therefore ends as SSDHIP_E_LAUNCH (-3) and a refused one as SSDHIP_E_BADARG (-1) or SSDHIP_E_WORKSPACE (-2), whatever the addresses:
they are made up here (16-byte aligned, never dereferenced) and must never reach a machine where a launch could run.

A case is a plain record: the entry, the arguments that differ from the entry's valid base call (a pointer as a byte offset from its
made-up aligned address or None for null, a host array as a list) and, for a few, environment variables.  Its id spells all of that
out, so tests/conv_entry_verdicts.json -- id -> return code, written once on the commit it names -- is readable on its own.

    CONV_ENTRY_RECORD=<commit hash> SSDHIP_LIB=<that commit's libssdhip.so> pytest tests/test_conv_entry_cpu.py

writes the file instead of comparing against it.
"""
import ctypes
import json
import os

from ssd_keras_amd import _native as nat

VERDICTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "conv_entry_verdicts.json")
RECORD_ENV = "CONV_ENTRY_RECORD"             # set to the hash of the commit under test: the test then WRITES the verdict file

LIM = 0x7ffff000                             # the 31-bit byte-offset limit of buffer addressing (refused from this value on)
_BASE, _STEP = 1 << 28, 1 << 24              # pointer argument number s of a call is the made-up address _BASE + s * _STEP

# Argument kinds: "p" device pointer (value: byte offset from its made-up address, None = null), "i" int, "f" float, "z" size_t,
# "P" HOST array of device pointers (list of offsets / None, or None for a null array), "I" HOST array of ints, "L" HOST array of
# long long (element strides; None for a null array).
_CONV = [("x", "p", 0), ("weight", "p", 0), ("bias", "p", 0), ("y", "p", 0), ("B", "i", 2), ("H", "i", 9), ("W", "i", 7)]
_SAME = _CONV + [("Cin", "i", 64), ("Cout", "i", 64), ("kernel", "i", 3), ("dilation", "i", 1), ("relu", "i", 1)]
_GENERAL = _CONV + [("Cin", "i", 64), ("Cout", "i", 64), ("kernel", "i", 3), ("stride", "i", 1), ("pad", "i", 1), ("dilation", "i", 1),
                    ("relu", "i", 1)]
_HALO = _CONV + [("Cin", "i", 128), ("Cout", "i", 128)]
_IMAGE = [("x", "p", 0), ("weight", "p", 0), ("bias", "p", 0), ("y", "p", 0), ("B", "i", 2), ("H", "i", 9), ("W", "i", 7)]
_GROUP = [("n_problems", "i", 2), ("x", "P", [0, 0]), ("weight", "P", [0, 0]), ("bias", "P", [0, 0]), ("y", "P", [0, 0]),
          ("B", "I", [2, 1]), ("H", "I", [9, 5]), ("W", "I", [7, 6])]

ENTRIES = {
    "ssdhip_conv2d_same_nhwc_bf16": _SAME,
    "ssdhip_conv2d_same_nhwc_bf16_variant": [("variant", "i", 4)] + _SAME,
    "ssdhip_conv2d_same_pool2_nhwc_bf16": _SAME,
    "ssdhip_conv2d_nhwc_bf16": _GENERAL,
    "ssdhip_conv2d_nhwc_bf16_variant": [("variant", "i", 4)] + _GENERAL,
    "ssdhip_conv2d_splitk_nhwc_bf16": _GENERAL + [("ksplit", "i", 2), ("ws", "p", 0), ("ws_bytes", "z", 2 * 2 * 9 * 7 * 64 * 4)],
    "ssdhip_conv2d_x3_nhwc_f16": _CONV + [("C", "i", 64), ("Cout", "i", 64), ("kernel", "i", 3), ("stride", "i", 1), ("pad", "i", 1),
                                          ("dilation", "i", 1), ("relu", "i", 1), ("pool", "i", 0), ("out_f32", "i", 0),
                                          ("oscale", "f", 4.0)],
    "ssdhip_conv2d_same_group_nhwc_bf16": _GROUP + [("Cin", "I", [64, 128]), ("Cout", "I", [64, 128]), ("kernel", "I", [3, 1]),
                                                    ("dilation", "I", [1, 2]), ("relu", "i", 1)],
    "ssdhip_conv3x3_cin3_nhwc_bf16": _CONV + [("Cin", "i", 3), ("Cout", "i", 64), ("relu", "i", 1)],
    "ssdhip_conv3x3_halo_nhwc_bf16": _HALO + [("relu", "i", 1), ("pool", "i", 0)],
    "ssdhip_conv3x3_halo_strided_nhwc_bf16": _HALO + [("stride", "i", 2), ("pad", "i", 1), ("relu", "i", 1)],
    "ssdhip_conv3x3_halo_group_nhwc_bf16": _GROUP + [("Cin", "I", [128, 256]), ("Cout", "I", [128, 256]), ("relu", "i", 1),
                                                     ("max_workgroups", "i", 0)],
    "ssdhip_conv3x3_halo_x3_nhwc_f16": _CONV + [("C", "i", 128), ("Cout", "i", 128), ("relu", "i", 1), ("pool", "i", 0),
                                                ("oscale", "f", 4.0)],
    # bias_rows 32: one tile of the 2 x 10 x 8 position grid per channel tile -> 8 workgroups of 4 wave rows (the query agrees, below)
    "ssdhip_conv3x3_halo_masked_nhwc_bf16": [("x", "p", 0), ("weight", "p", 0), ("mask", "p", 0), ("y", "p", 0), ("bias_partial", "p", 0),
                                             ("bias_rows", "i", 32), ("B", "i", 2), ("H", "i", 9), ("W", "i", 7), ("Cin", "i", 128),
                                             ("Cout", "i", 128)],
    "ssdhip_conv3x3_halo_pool_keep_nhwc_bf16": [("x", "p", 0), ("weight", "p", 0), ("bias", "p", 0), ("y_full", "p", 0),
                                                ("y_pooled", "p", 0), ("B", "i", 2), ("H", "i", 9), ("W", "i", 7), ("Cin", "i", 128),
                                                ("Cout", "i", 128), ("relu", "i", 1)],
    "ssdhip_conv2d_image_nhwc_bf16": _IMAGE + [("Cin", "i", 64), ("Cout", "i", 64), ("ksize", "i", 3), ("stride", "i", 1),
                                               ("pad", "i", 1), ("dilation", "i", 1), ("relu", "i", 1)],
    "ssdhip_conv2d_image_x3_nhwc_f16": _IMAGE + [("C", "i", 64), ("Cout", "i", 64), ("ksize", "i", 3), ("stride", "i", 1), ("pad", "i", 1),
                                                 ("dilation", "i", 1), ("relu", "i", 1), ("out_f32", "i", 0), ("oscale", "f", 4.0)],
    "ssdhip_conv3x3_image_nhwc_bf16": _IMAGE + [("Cin", "i", 64), ("Cout", "i", 64), ("dilation", "i", 1), ("relu", "i", 1)],
    "ssdhip_conv3x3_c64_nhwc_bf16": _CONV + [("Cin", "i", 64), ("Cout", "i", 64), ("relu", "i", 1), ("pool", "i", 0),
                                             ("n_workgroups", "i", 0)],
    "ssdhip_conv3x3_c64_pool_keep_nhwc_bf16": [("x", "p", 0), ("weight", "p", 0), ("bias", "p", 0), ("y_full", "p", 0),
                                               ("y_pooled", "p", 0), ("B", "i", 2), ("H", "i", 9), ("W", "i", 7), ("Cin", "i", 64),
                                               ("Cout", "i", 64), ("relu", "i", 1), ("n_workgroups", "i", 0)],
    "ssdhip_conv1_block_nhwc_bf16": [("x3", "p", 0), ("w1", "p", 0), ("b1", "p", 0), ("weight", "p", 0), ("bias", "p", 0), ("y", "p", 0),
                                     ("B", "i", 2), ("H", "i", 9), ("W", "i", 7), ("Cout", "i", 64), ("relu", "i", 1), ("pool", "i", 0),
                                     ("n_workgroups", "i", 0)],
}


def _dense(cout, cin, k):
    """element strides (Cout, Cin, kh, kw) of a contiguous (Cout, Cin, k, k) parameter"""
    return [cin * k * k, k * k, k, 1]


# --- the SSD7 family (csrc/ssdhip_convbn.hip, ssdhip_wgrad7.hip, ssdhip_heads7.hip).  The weight gradients' base workspace is larger
# than any perturbation of the base call needs; the exact sizes are cases of their own (_special)
SSD7_GEOMETRIES = ((32, 48, 3), (48, 64, 3), (48, 48, 3), (48, 32, 3), (64, 64, 3), (64, 48, 3), (3, 32, 5))
_MAP7 = [("B", "i", 2), ("H", "i", 9), ("W", "i", 7)]
SSD7_ENTRIES = ("ssdhip_conv_bn_elu_nhwc_bf16", "ssdhip_conv_same_bias_nhwc_bf16", "ssdhip_ssd7_pack_filters", "ssdhip_ssd7_pack_heads",
                "ssdhip_ssd7_conv_wgrad_nhwc_bf16", "ssdhip_ssd7_head_wgrad_nhwc_bf16")
ENTRIES.update({
    "ssdhip_conv_bn_elu_nhwc_bf16": [("x", "p", 0), ("w_packed", "p", 0), ("scale", "p", 0), ("shift", "p", 0), ("y", "p", 0)] + _MAP7 +
                                    [("Cin", "i", 64), ("Cout", "i", 64), ("kernel", "i", 3), ("pool", "i", 0)],
    "ssdhip_conv_same_bias_nhwc_bf16": [("x", "p", 0), ("w_packed", "p", 0), ("bias", "p", 0), ("y", "p", 0)] + _MAP7 +
                                       [("Cin", "i", 64), ("Cout", "i", 64), ("kernel", "i", 3)],
    "ssdhip_ssd7_pack_filters": [("n_layers", "i", 2), ("weights", "P", [0, 0]), ("fwd", "P", [0, 0]), ("flipped", "P", [0, 0]),
                                 ("Cin", "I", [64, 48]), ("Cout", "I", [64, 32]), ("kernel", "I", [3, 3]),
                                 ("strides", "L", _dense(64, 64, 3) + _dense(32, 48, 3))],
    "ssdhip_ssd7_pack_heads": [("n_maps", "i", 2)] + [(n, "P", [0, 0]) for n in ("conf_w", "loc_w", "conf_b", "loc_b", "fwd", "flipped", "bias")] +
                              [("Cin", "I", [64, 48]), ("n_conf", "I", [24, 20]), ("n_loc", "I", [16, 16]),
                               ("strides", "L", _dense(24, 64, 3) + _dense(16, 64, 3) + _dense(20, 48, 3) + _dense(16, 48, 3))],
    "ssdhip_ssd7_conv_wgrad_nhwc_bf16": [("x", "p", 0), ("dy", "p", 0), ("dw", "p", 0), ("db", "p", 0)] + _MAP7 +
                                        [("Cin", "i", 64), ("Cout", "i", 64), ("kernel", "i", 3), ("out_bf16", "i", 0),
                                         ("dw_strides", "L", _dense(64, 64, 3)), ("workspace", "p", 0), ("workspace_bytes", "z", 1 << 20)],
    "ssdhip_ssd7_head_wgrad_nhwc_bf16": [("x", "p", 0), ("dy", "p", 0), ("dw_conf", "p", 0), ("db_conf", "p", 0), ("dw_loc", "p", 0),
                                         ("db_loc", "p", 0)] + _MAP7 +
                                        [("Cin", "i", 64), ("Cp", "i", 48), ("n_conf", "i", 24), ("n_loc", "i", 16), ("out_bf16", "i", 0),
                                         ("dw_conf_strides", "L", _dense(24, 64, 3)), ("dw_loc_strides", "L", _dense(16, 64, 3)),
                                         ("workspace", "p", 0), ("workspace_bytes", "z", 1 << 20)],
})

CHANNELS = (0, -1, 1, 32, 48, 64, 96, 128, 192)
DIMS = (0, -1, 1)
_VALUES = {"B": DIMS, "H": DIMS, "W": DIMS, "Cin": CHANNELS, "C": CHANNELS, "Cout": CHANNELS, "kernel": (0, 1, 2, 3, 5),
           "ksize": (0, 1, 2, 3, 5), "stride": (0, 1, 2, 3, 4, 5), "dilation": (0, 1, 8, 9, 16, 17), "relu": (0, 2), "pool": (0, 1, 2),
           "out_f32": (0, 1), "n_workgroups": (-1, 1, 3, 8, 256, 5000), "max_workgroups": (-1, 7, 8, 64), "variant": tuple(range(0, 10)),
           "n_problems": (0, -1, 1), "ksplit": (0, -1, 1, 9, 10, 1000), "oscale": (0.0, -1.0, 1.0, float("nan")),
           "bias_rows": (31, 33, 0), "Cp": CHANNELS, "n_conf": (0,), "n_loc": (0,), "out_bf16": (0, 1)}


def _below(limit, per, const=0):
    """the largest n with n * per + const < limit"""
    return (limit - const - 1) // per


def _generic(entry):
    """One-at-a-time perturbations of every argument of `entry`'s base call."""
    spec = ENTRIES[entry]
    base = {n: v for n, _, v in spec}
    group = "n_problems" in base
    out = []
    for name, kind, _ in spec:
        if kind == "p":
            out += [{name: v} for v in (None, 1, 2, 4, 8)]               # (1: the 2-byte rule of a bf16 bias)
        elif kind == "P":                                  # the array itself null; its second problem's pointer null / misaligned
            out += [{name: None}] + [{name: [0, v]} for v in (None, 1, 2, 4, 8)]
        elif kind == "I":
            out += [{name: None}] + [{name: [base[name][0], v]} for v in _VALUES.get(name, ()) if v != base[name][1]]
        elif kind == "L":                                  # the array null (dense, where the entry allows it); one negative stride
            out += [{name: None}, {name: [-1] + base[name][1:]}]
        else:
            out += [{name: v} for v in _VALUES.get(name, ()) if v != base[name]]
    if "pad" in base and "stride" in base and "halo" not in entry:
        kname = "ksize" if "ksize" in base else "kernel"
        # pad against the filter's reach (k = 3, dilation 2: reach 2; k = 1: reach 0); every dilation as a 'same' call and at pad 0
        out += [{"dilation": 2, "pad": v} for v in (-1, 0, 1, 2, 3)] + [{kname: 1, "pad": v} for v in (-1, 0, 1)]
        out += [{"dilation": d, "pad": d, "H": 19, "W": 19} for d in _VALUES["dilation"]]
        out += [{"dilation": d, "pad": 0, "H": 19, "W": 19} for d in (1, 8, 9, 10)]
        # H + 2 pad against the filter span 2 reach + 1
        out += [{"pad": 0, "H": h} for h in (2, 3)] + [{"pad": 0, "W": w} for w in (2, 3)] + [{"pad": 1, "dilation": 2, "H": h} for h in (2, 3)]
        out += [{"stride": s, "pad": 0, "H": 3, "W": 3} for s in (2, 4)]
    elif "dilation" in base and not group:
        out += [{"dilation": d, "H": 19, "W": 19} for d in _VALUES["dilation"]]
    if "pad" in base and "halo" in entry:                  # the strided slab form: stride 1 | 2, pad 0 | 1, the 3 x 3 span, W <= 94
        out += [{"pad": v} for v in (-1, 0, 2)] + [{"stride": s, "pad": p_} for s in (1, 2) for p_ in (0, 1)]
        out += [{"pad": 0, "H": h} for h in (2, 3)] + [{"pad": 0, "W": w} for w in (2, 3)] + [{"pad": 1, "H": 1, "W": 1}]
    if not group and "W" in base and "image" not in entry and entry not in SSD7_ENTRIES:
        out += [{"W": w} for w in (30, 31, 62, 63, 94, 95)]
    return out


def _special():
    """The checks a one-at-a-time perturbation of the small base call does not reach, by entry."""
    c = []

    def add(entry, **kw):
        env = kw.pop("env", None)
        c.append((entry, kw, env))

    same, samev, pool2 = "ssdhip_conv2d_same_nhwc_bf16", "ssdhip_conv2d_same_nhwc_bf16_variant", "ssdhip_conv2d_same_pool2_nhwc_bf16"
    gen, genv, splitk = "ssdhip_conv2d_nhwc_bf16", "ssdhip_conv2d_nhwc_bf16_variant", "ssdhip_conv2d_splitk_nhwc_bf16"
    x3, grp = "ssdhip_conv2d_x3_nhwc_f16", "ssdhip_conv2d_same_group_nhwc_bf16"
    # --- ssdhip_conv.hip: input bytes M Cin 2 + 4 (dil W + dil) Cin < LIM (64 channels, W = 1: M 128 + 512), on both sides.  Beyond it
    # the 'same' entries hand variants 4 / 5 / 6 to variant 1 (64-bit addressing) and the others refuse
    m_in = _below(LIM, 128, 512)
    for h in (m_in, m_in + 1):
        for e in (same, pool2, gen):
            add(e, B=1, H=h, W=1)
        add(splitk, B=1, H=h, W=1, ksplit=1, ws_bytes=1 << 62)
        for v in (1, 4, 5, 6):
            add(samev, variant=v, B=1, H=h, W=1)
        for v in (4, 5, 6):
            add(genv, variant=v, B=1, H=h, W=1)
        add(grp, B=[2, 1], H=[9, h], W=[7, 1], Cin=[64, 64], Cout=[64, 64], kernel=[3, 3], dilation=[1, 1])
    add(same, B=1, H=1 << 24, W=1, Cin=64)                # 2 GiB of input: variant 4 becomes variant 1
    add(same, B=4, H=4096, W=4096, Cin=128, Cout=128)     # 32 GiB
    # variant 1's own limit: M max(Cin, Cout) <= 0x7fffffff0
    m_idx = 0x7fffffff0 // 64
    for h in (m_idx, m_idx + 1):
        add(same, B=1, H=h, W=1)
        add(samev, variant=1, B=1, H=h, W=1)
    # filter bytes Cout k k Cin 2 < LIM (3 x 3: Cin Cout < LIM / 18: 170 x 64 squared inside, 171 x 64 outside)
    for ch in (170 * 64, 171 * 64):
        for e in (same, pool2, gen):
            add(e, Cin=ch, Cout=ch)
        add(splitk, Cin=ch, Cout=ch, ksplit=1, ws_bytes=1 << 62)
        add(grp, Cin=[64, ch], Cout=[64, ch], kernel=[3, 3])
    # output index M Cout <= 0x7fffffff0 of the general forms (1 x 1 on W = 1, 33 x 64 output channels)
    m_out = 0x7fffffff0 // 2112
    for h in (m_out, m_out + 1):
        add(gen, B=1, H=h, W=1, kernel=1, pad=0, Cout=2112)
        add(splitk, B=1, H=h, W=1, kernel=1, pad=0, Cout=2112, ksplit=1, ws_bytes=1 << 62)
        add(grp, B=[2, 1], H=[9, h], W=[7, 1], Cin=[64, 64], Cout=[64, 2112], kernel=[3, 1], dilation=[1, 1])
    # pooled tiles B HT WT <= 0x3fffffff / n_tiles (1 x 1 maps: one tile per image; 100 channel tiles)
    t_max = 0x3fffffff // 100
    for b in (t_max, t_max + 1):
        add(pool2, B=b, H=1, W=1, Cout=12800)
    # the X3 form: input rows of 2 C float16, filters of 3 C, M Cout <= 0x3fffffff0
    m_x3 = _below(LIM, 256, 1024)
    for h in (m_x3, m_x3 + 1):
        add(x3, B=1, H=h, W=1)
    for ch in (98 * 64, 99 * 64):                         # Cout 9 (3 C) 2 < LIM: C Cout < LIM / 54
        add(x3, C=ch, Cout=ch)
    m_x3o = 0x3fffffff0 // 2112
    for h in (m_x3o, m_x3o + 1):
        add(x3, B=1, H=h, W=1, kernel=1, pad=0, Cout=2112)
    # (the X3 form's own pooled-tile limit and the group forms' block limits lie beyond their M Cout / byte limits: no call reaches them)
    # X3 pooling is the stride-1 'same' form only; either output format; the pooled tile search on an odd map
    for kw in ({"pool": 1, "stride": 2}, {"pool": 1, "pad": 0}, {"pool": 1, "kernel": 1, "pad": 0}, {"pool": 1, "out_f32": 1},
               {"pool": 1, "H": 75, "W": 75, "Cout": 128}, {"pool": 1, "dilation": 2, "pad": 2}, {"pool": 1, "dilation": 2, "pad": 1}):
        add(x3, **kw)
    # split-K: ksplit against the K steps (k k Cin / 64 = 9 here: more is clamped), the workspace one float short, 0 = chosen by the entry
    per = 2 * 9 * 7 * 64 * 4                              # one float32 copy of the base call's output
    for ks, ws in ((1, per), (1, per - 1), (2, 2 * per - 1), (9, 9 * per), (9, 9 * per - 1), (10, 9 * per), (10, 9 * per - 1), (0, 9 * per),
                   (0, 9 * per - 1), (0, 0), (-3, 9 * per)):
        add(splitk, ksplit=ks, ws_bytes=ws)
    add(splitk, kernel=1, pad=0, ksplit=2, ws_bytes=per)       # one K step: clamped to 1
    add(splitk, kernel=1, pad=0, ksplit=2, ws_bytes=per - 1)
    add(splitk, stride=2, ksplit=1, ws_bytes=2 * 5 * 4 * 64 * 4)
    add(splitk, stride=2, ksplit=1, ws_bytes=2 * 5 * 4 * 64 * 4 - 1)
    add(splitk, bias=None, ws=None)
    # the group forms: 1, the maximum and one more problem; a later problem refused; the bias array absent
    for e, chan in ((grp, {"kernel": [3] * 9, "dilation": [1] * 9}), ("ssdhip_conv3x3_halo_group_nhwc_bf16", {})):
        c0 = 64 if e == grp else 128
        for n in (1, 8, 9):
            add(e, n_problems=n, x=[0] * 9, weight=[0] * 9, bias=[0] * 9, y=[0] * 9, B=[1] * 9, H=[5] * 9, W=[6] * 9, Cin=[c0] * 9,
                Cout=[c0] * 9, **chan)
        add(e, n_problems=8, x=[0] * 7 + [None], weight=[0] * 8, bias=[0] * 8, y=[0] * 8, B=[1] * 8, H=[5] * 8, W=[6] * 8, Cin=[c0] * 8,
            Cout=[c0] * 8, **{k: v[:8] for k, v in chan.items()})
        add(e, bias=[None, None])
        for w in (62, 63, 94, 95):
            add(e, W=[7, w])
            add(e, W=[w, 6])
    # --- ssdhip_convh.hip: x / filter / y bytes < LIM (128 channels: 256 bytes per pixel)
    halo, strided, hx3 = "ssdhip_conv3x3_halo_nhwc_bf16", "ssdhip_conv3x3_halo_strided_nhwc_bf16", "ssdhip_conv3x3_halo_x3_nhwc_f16"
    masked, keep, hgrp = "ssdhip_conv3x3_halo_masked_nhwc_bf16", "ssdhip_conv3x3_halo_pool_keep_nhwc_bf16", "ssdhip_conv3x3_halo_group_nhwc_bf16"
    px = _below(LIM, 256)
    for h in (px, px + 1):
        for e in (halo, strided, keep):
            add(e, B=1, H=h, W=1)
        add(halo, B=1, H=h, W=1, pool=1)
        add(masked, B=1, H=h, W=1, bias_partial=None)
        add(hgrp, B=[2, 1], H=[9, h], W=[7, 1], Cin=[128, 128], Cout=[128, 128])
    pxo = _below(LIM, 512)                                # the output map's bytes with 256 channels
    for h in (pxo, pxo + 1):
        for e in (halo, strided, keep):
            add(e, B=1, H=h, W=1, Cout=256)
        add(halo, B=1, H=h, W=1, Cout=256, pool=1)         # (the pooled output is a quarter: the limit is on the full-size map)
        add(masked, B=1, H=h, W=1, Cout=256, bias_partial=None)
        add(hgrp, B=[2, 1], H=[9, h], W=[7, 1], Cin=[128, 128], Cout=[128, 256])
    for ch in (85 * 128, 86 * 128):                       # Cout 9 Cin 2 < LIM
        for e in (halo, strided, keep):
            add(e, Cin=ch, Cout=ch)
        add(masked, Cin=ch, Cout=ch, bias_partial=None)       # (85 channel tiles: refused, no grid of 256 workgroups is a multiple of 8 x 85)
        add(hgrp, Cin=[128, ch], Cout=[128, ch])
    for ch in (227 * 128, 228 * 128):                     # the same limit with 32 channel tiles
        add(masked, Cin=ch, Cout=4096, bias_partial=None)
    add(masked, Cout=4096 + 128, bias_partial=None)       # 33 channel tiles: 8 x 33 workgroups > 256
    pxx = _below(LIM, 512)                                # X3: rows of 2 C float16 in, 2 Cout float16 out
    for h in (pxx, pxx + 1):
        add(hx3, B=1, H=h, W=1)
        add(hx3, B=1, H=h, W=1, pool=1)
    for ch in (49 * 128, 50 * 128):                       # Cout 9 (3 C) 2 < LIM
        add(hx3, C=ch, Cout=ch)
    add(hx3, C=64)                                        # conv2_1: three 64-channel slices padded to four
    add(hx3, C=64, pool=1)
    # maps: the pooled forms on 2-D tiles (stacked or per image), the un-pooled ones on the grid or on 2-D tiles beyond 94 columns
    for e in (halo, hx3):
        for kw in ({"pool": 1}, {"pool": 1, "H": 75, "W": 75, "B": 32}, {"H": 64, "W": 64, "B": 16, "Cout": 512}, {"H": 150, "W": 150},
                   {"pool": 1, "H": 150, "W": 150}):
            add(e, **kw)
    for mode in ("128", "1152", "0"):
        add(halo, pool=1, H=75, W=75, B=32, env={"SSDHIP_CONVH_MODE": mode})
    add(halo, H=64, W=64, B=16, Cout=512, env={"SSDHIP_CONVH_GRID": "1"})
    add(halo, pool=1, H=75, W=75, B=32, env={"SSDHIP_CONVH_STACK": "0"})
    # the masked form's bias_rows against its grid: 16 x 64 x 64 x 512 runs on 2-D tiles (256 x 4 units, one workgroup per CU of 256)
    for rows in (255, 256, 257):
        add(masked, B=16, H=64, W=64, Cout=512, bias_rows=rows)
    add(masked, B=16, H=64, W=64, Cout=512, bias_rows=256, env={"SSDHIP_CONVH_GRID": "1"})
    add(masked, B=16, H=64, W=64, Cout=512, bias_rows=272, env={"SSDHIP_CONVH_GRID": "1"})
    add(masked, bias_partial=None, bias_rows=7)            # not checked without a table
    add(masked, H=150, W=150, bias_partial=None)
    # --- ssdhip_convimg.hip: 384 pixels in and out, the filter span, bytes of one image and of a filter tile
    img, img3, img33 = "ssdhip_conv2d_image_nhwc_bf16", "ssdhip_conv2d_image_x3_nhwc_f16", "ssdhip_conv3x3_image_nhwc_bf16"
    for e in (img, img3):
        for kw in ({"H": 16, "W": 24}, {"H": 35, "W": 11}, {"H": 1, "W": 385}, {"H": 19, "W": 19, "dilation": 6, "pad": 6},
                   {"H": 20, "W": 20}, {"H": 18, "W": 20, "pad": 1}, {"H": 18, "W": 20, "pad": 1, "ksize": 1},   # 360 in, 400 out
                   {"H": 20, "W": 20, "stride": 2}, {"H": 20, "W": 20, "ksize": 1, "pad": 0, "stride": 2},       # 400 in, 100 out
                   {"H": 19, "W": 19, "ksize": 1, "pad": 0}, {"H": 19, "W": 19, "ksize": 1, "pad": 0, "Cin" if e == img else "C": 1024, "Cout": 256},
                   {"B": 32, "H": 19, "W": 19, "ksize": 1, "pad": 0, "Cout": 1024}, {"B": 8, "Cout": 128}):
            add(e, **kw)
    for d in (1, 6, 16, 17):
        add(img33, H=19, W=19, dilation=d)
    add(img33, H=20, W=20)
    for ch in (43690 * 64, 43691 * 64):                   # H W max(Cin, Cout) 2 < LIM at 384 pixels
        add(img, H=16, W=24, Cout=ch)
    for ch in (14563 * 64, 14564 * 64):                   # a filter tile: 128 x 9 x Cin x 2 < LIM
        add(img, H=1, W=1, ksize=1, pad=0, Cin=ch)
    for ch in (7281 * 64, 7282 * 64):                     # X3: H W 3 max(C, Cout) 4 < LIM at 384 pixels
        add(img3, H=16, W=24, Cout=ch)
    for ch in (4854 * 64, 4855 * 64):                     # X3: 128 x 9 x 3 C x 2 < LIM
        add(img3, H=1, W=1, ksize=1, pad=0, C=ch)
    add(img3, out_f32=1, bias=None)
    # --- ssdhip_conv64.hip: x bytes B H W 128 < LIM, filters Cout 1152 < LIM, B H W Cout <= 0x7fffffff0; y2 needs pool
    c64, c64k, c1b = "ssdhip_conv3x3_c64_nhwc_bf16", "ssdhip_conv3x3_c64_pool_keep_nhwc_bf16", "ssdhip_conv1_block_nhwc_bf16"
    p64 = _below(LIM, 128)
    for h in (p64, p64 + 1):
        for e in (c64, c64k):
            add(e, B=1, H=h, W=1)
        add(c64, B=1, H=h, W=1, pool=1)
    p3 = _below(LIM, 6)                                   # the fused first block reads the 3-channel image: 6 bytes per pixel
    for h in (p3, p3 + 1):
        add(c1b, B=1, H=h, W=1)
        add(c1b, B=1, H=h, W=1, pool=1)
    for co in (_below(LIM, 1152) // 64 * 64, _below(LIM, 1152) // 64 * 64 + 64):
        for e in (c64, c64k, c1b):
            add(e, Cout=co)
    for e in (c64, c64k, c1b):
        m = 0x7fffffff0 // 4096
        for h in (m, m + 1):
            add(e, B=1, H=h, W=1, Cout=4096)
        for kw in ({"H": 300, "W": 300}, {"H": 8, "W": 33}, {"Cout": 128, "n_workgroups": 256}, {"Cout": 128, "n_workgroups": 250}):
            add(e, **kw)
    add(c64, pool=1, H=300, W=300)
    add(c1b, pool=1, H=300, W=300)
    for prio in ("0", "1", "3"):
        add(c64, env={"SSDHIP_C64_PRIO": prio})
        add(c1b, env={"SSDHIP_C64_PRIO": prio})
    add(c64, Cout=128, n_workgroups=256, env={"SSDHIP_C64_XCD": "0"})
    # --- the first layer
    cin3 = "ssdhip_conv3x3_cin3_nhwc_bf16"
    for h in (0x7fffff00, 0x7fffff01):
        add(cin3, B=1, H=h, W=1)
    add(cin3, H=300, W=300, B=32)
    # variant 7 of the 'same' profiling entry is the slab kernel: 3 x 3, dilation 1, 128-channel multiples
    for kw in ({"Cin": 128, "Cout": 128}, {"Cin": 128, "Cout": 128, "kernel": 1}, {"Cin": 128, "Cout": 128, "dilation": 2}, {}):
        add(samev, variant=7, **kw)
    # --- the SSD7 family: each of the seven geometries once per entry; beside them the swapped pair, which is none
    cbn, cbias, packf, packh = "ssdhip_conv_bn_elu_nhwc_bf16", "ssdhip_conv_same_bias_nhwc_bf16", "ssdhip_ssd7_pack_filters", "ssdhip_ssd7_pack_heads"
    w7, h7 = "ssdhip_ssd7_conv_wgrad_nhwc_bf16", "ssdhip_ssd7_head_wgrad_nhwc_bf16"
    for ci, co, k in SSD7_GEOMETRIES + ((32, 3, 5), (48, 3, 3)):
        add(cbn, Cin=ci, Cout=co, kernel=k, pool=1)
        add(cbias, Cin=ci, Cout=co, kernel=k)
        add(w7, Cin=ci, Cout=co, kernel=k, dw_strides=_dense(co, ci, k))
        add(packf, Cin=[64, ci], Cout=[64, co], kernel=[3, k], strides=_dense(64, 64, 3) + _dense(co, ci, k), flipped=[0, None])
    add(packf, Cin=[64, 3], Cout=[64, 32], kernel=[3, 5], strides=_dense(64, 64, 3) + _dense(32, 3, 5))    # a flipped image of the 5 x 5 layer
    add(packf, flipped=[None, None])
    for e in (cbn, cbias, w7):                            # the 5 x 5 layer reads x at 2-byte alignment
        add(e, Cin=3, Cout=32, kernel=5, x=2)
        add(e, Cin=3, Cout=32, kernel=5, x=1)
    for kw in ({"H": 1}, {"W": 1}, {"H": 2, "W": 2}):
        add(cbn, pool=1, **kw)
    add(cbn, pool=0, H=1, W=1)
    # the position limits: B H W (and with it the tile count) <= 0x3fffffff; the heads' padded list B (H + 2)(W + 2) likewise
    for b in (0x3fffffff, 0x40000000):
        for e in (cbn, cbias):
            add(e, B=b, H=1, W=1)
        add(w7, B=b, H=1, W=1, workspace_bytes=1 << 62)
    for b in (0x3fffffff // 9, 0x3fffffff // 9 + 1):
        add(h7, B=b, H=1, W=1, workspace_bytes=1 << 62)
    for w in (255, 256, 257):                             # the head kernel keeps 256 + 2 (W + 3) rows in LDS: W <= 256
        add(h7, W=w, workspace_bytes=1 << 62)
    # the workspaces: exact and one byte short.  Base calls: one split of (64 x 9 x 64 + 64) / (48 x 9 x 64 + 48) floats; Cin = 32 heads
    # keep two step-parity partials; 8 x 40 x 70 at (48, 64) splits 20 ways, the heads' 32 x 37 x 37 64 ways
    for e, kw, need in ((w7, {}, 147712), (w7, {"B": 8, "H": 40, "W": 70, "Cin": 48}, 20 * 110848), (h7, {}, 110784),
                        (h7, {"Cin": 32}, 2 * 55488), (h7, {"B": 32, "H": 37, "W": 37}, 64 * 110784)):
        for n in (need, need - 1):
            add(e, workspace_bytes=n, **kw)
    # outputs at 2-byte alignment: bf16 only
    for bf in (1, 0):
        add(w7, out_bf16=bf, dw=2, db=2)
        add(h7, out_bf16=bf, dw_conf=2, db_conf=2, dw_loc=2, db_loc=2)
    add(w7, db=None, out_bf16=1)
    # element strides: zero is allowed; the farthest element they address (Cin = 64: 63 s1 + 2 s2) at 0x3fffffff and one past it
    at, past = [0, 0x3fffffff // 63, 0, 0], [0, 0x3fffffff // 63 - 1, 32, 0]
    for s in (at, past, [0, 0, 0, 0]):
        add(w7, dw_strides=s)
        add(h7, dw_conf_strides=s)
        add(h7, dw_loc_strides=s)
        add(packf, strides=s + _dense(32, 48, 3))
        add(packh, strides=_dense(24, 64, 3) + s + _dense(20, 48, 3) + _dense(16, 48, 3))
    add(packf, strides=_dense(64, 64, 3) + [5, 5, -5, 5])
    add(packh, strides=_dense(24, 64, 3) + _dense(16, 64, 3) + _dense(20, 48, 3) + [1, 1, 1, -1])
    add(h7, dw_conf_strides=None, dw_loc_strides=None)
    # the heads' rows: n_conf + n_loc <= 48
    for nc, nl in ((24, 24), (25, 24), (47, 1), (48, 1), (-1, 16)):
        add(h7, n_conf=nc, n_loc=nl)
        add(packh, n_conf=[24, nc], n_loc=[16, nl])
    # the tables: 1, the maximum and one more layer / map; a later layer's pointer missing
    for n in (0, 1, 8, 9):
        add(packf, n_layers=n, weights=[0] * 9, fwd=[0] * 9, flipped=[0] * 9, Cin=[64] * 9, Cout=[64] * 9, kernel=[3] * 9,
            strides=_dense(64, 64, 3) * 9)
        add(packh, n_maps=n, Cin=[64] * 9, n_conf=[24] * 9, n_loc=[16] * 9, strides=_dense(24, 64, 3) * 18,
            **{name: [0] * 9 for name in ("conf_w", "loc_w", "conf_b", "loc_b", "fwd", "flipped", "bias")})
    add(packf, n_layers=8, weights=[0] * 7 + [None], fwd=[0] * 8, flipped=[0] * 8, Cin=[64] * 8, Cout=[64] * 8, kernel=[3] * 8,
        strides=_dense(64, 64, 3) * 8)
    return c


def _case_id(entry, over, env):
    def show(v):
        return repr(v).replace(" ", "")
    cid = entry + "|" + ",".join("%s=%s" % (k, show(over[k])) for k in sorted(over))
    if env:
        cid += "|" + ",".join("%s=%s" % kv for kv in sorted(env.items()))
    return cid


def cases():
    """id -> (entry, overrides, environment)"""
    out = {}
    for entry in ENTRIES:
        out[_case_id(entry, {}, None)] = (entry, {}, None)
        for over in _generic(entry):
            out[_case_id(entry, over, None)] = (entry, over, None)
    for entry, over, env in _special():
        out[_case_id(entry, over, env)] = (entry, over, env)
    return out


# The host-only queries: (export, arguments, environment)
def queries():
    q = {}

    def add(name, args, env=None):
        q[_case_id(name, {"args": list(args)}, env)] = (name, tuple(args), env)

    for geo in ((2, 9, 7, 64, 64, 3, 1, 1, 1), (2, 9, 7, 64, 64, 3, 2, 1, 1), (2, 9, 7, 64, 64, 1, 1, 0, 1), (32, 10, 10, 128, 256, 3, 2, 1, 1),
                (32, 19, 19, 1024, 256, 1, 1, 0, 1), (32, 3, 3, 128, 256, 3, 1, 0, 1), (1, 300, 300, 64, 128, 3, 1, 1, 1),
                (2, 9, 7, 48, 64, 3, 1, 1, 1), (2, 9, 7, 64, 96, 3, 1, 1, 1), (2, 9, 7, 64, 64, 2, 1, 1, 1), (2, 9, 7, 64, 64, 3, 5, 1, 1),
                (2, 9, 7, 64, 64, 3, 1, 2, 1), (2, 9, 7, 64, 64, 3, 1, 1, 9), (2, 2, 7, 64, 64, 3, 1, 0, 1), (0, 9, 7, 64, 64, 3, 1, 1, 1),
                (2, 9, 7, 64, 64, 3, 1, -1, 1), (2, 9, 7, 64, 64, 3, 0, 1, 1), (2, 9, 7, 64, 64, 3, 1, 1, 0), (2, 9, 7, 64, 64, 3, 1, 8, 8)):
        for ks in (0, 1, 2, 9, 10, 1000):
            add("ssdhip_conv2d_splitk_workspace_bytes", geo + (ks,))
    plans = [(b, s, s, co, pool) for b in (1, 8, 16, 32) for s, co in ((300, 64), (150, 128), (75, 256), (38, 512), (19, 512), (64, 512),
                                                                      (128, 256), (32, 512)) for pool in (0, 1)]
    plans += [(2, 9, 7, 128, 0), (2, 9, 7, 128, 1), (1, 1, 1, 128, 0), (1, 1, 1, 128, 1), (1, 94, 94, 128, 0), (1, 95, 95, 128, 0),
              (0, 9, 7, 128, 0), (2, 0, 7, 128, 0), (2, 9, 0, 128, 0), (2, 9, 7, 0, 0), (2, 9, 7, 64, 0), (2, 9, 7, 192, 1),
              (1 << 20, 31, 31, 128, 0), (1 << 21, 31, 31, 128, 0), (1 << 22, 15, 15, 128, 0), (1 << 23, 15, 15, 128, 1), (1 << 30, 15, 15, 128, 1),
              (1 << 23, 200, 200, 128, 0)]
    for p_ in plans:
        add("ssdhip_conv3x3_halo_plan", p_)
    for p_ in plans[:64:3]:
        add("ssdhip_conv3x3_halo_plan", p_, {"SSDHIP_CONVH_GRID": "1"})
        add("ssdhip_conv3x3_halo_plan", p_, {"SSDHIP_CONVH_STACK": "0"})
    rows = [(b, s, s, co) for b in (1, 8, 16, 32) for s, co in ((150, 128), (75, 256), (38, 512), (64, 512), (19, 512))]
    rows += [(2, 9, 7, 128), (0, 9, 7, 128), (2, -1, 7, 128), (2, 9, 0, 128), (2, 9, 7, 64), (2, 9, 7, 0), (1, 200, 200, 128),
             (1 << 22, 15, 15, 128), (1 << 23, 200, 200, 128)]
    for r in rows:
        add("ssdhip_conv3x3_halo_masked_bias_rows", r)
    for r in rows[:20:3]:
        add("ssdhip_conv3x3_halo_masked_bias_rows", r, {"SSDHIP_CONVH_GRID": "1"})
    # the SSD7 family: the image size of the seven geometries and of their neighbours; the weight gradients' workspaces on the GPU
    # suites' maps for every geometry, their plans (several ints each) for one map per geometry, and the limits
    for geo in SSD7_GEOMETRIES + ((32, 3, 5), (48, 3, 3), (64, 32, 3), (32, 32, 3), (96, 64, 3), (64, 64, 1), (64, 64, 5), (0, 48, 3), (3, 32, 3)):
        add("ssdhip_conv_bn_elu_pack_bytes", geo)
    maps = [(3, 19, 37), (2, 10, 150), (1, 6, 480), (3, 40, 70), (8, 40, 70), (32, 300, 480), (32, 150, 240)]
    bad = [(0, 9, 7), (2, -1, 7), (2, 9, 0), (0x3fffffff, 1, 1), (0x40000000, 1, 1), (1 << 16, 1 << 8, 1 << 6)]
    for i, geo in enumerate(SSD7_GEOMETRIES):
        add("ssdhip_ssd7_conv_wgrad_plan", maps[i] + geo)
        for m in maps:
            add("ssdhip_ssd7_conv_wgrad_workspace_bytes", m + geo)
    for m in bad:                                         # (a refused plan is a line per int in the verdict file: two of them)
        add("ssdhip_ssd7_conv_wgrad_workspace_bytes", m + (64, 64, 3))
    for geo in ((64, 32, 3), (3, 32, 3)):
        add("ssdhip_ssd7_conv_wgrad_workspace_bytes", maps[0] + geo)
    add("ssdhip_ssd7_conv_wgrad_plan", bad[4] + (64, 64, 3))
    add("ssdhip_ssd7_conv_wgrad_plan", maps[0] + (64, 32, 3))
    maps = [(1, 4, 4), (8, 9, 9), (32, 18, 18), (32, 37, 37), (2, 9, 256), (512, 64, 256)]
    bad = [(2, 9, 257), (0, 9, 7), (2, 0, 7), (2, 9, -1), (0x3fffffff // 9, 1, 1), (0x3fffffff // 9 + 1, 1, 1)]
    for i, ci in enumerate((64, 48, 32)):
        for m in maps:
            add("ssdhip_ssd7_head_wgrad_workspace_bytes", m + (ci, 48))
        for m in (maps[i], maps[3]):
            add("ssdhip_ssd7_head_wgrad_plan", m + (ci, 48))
    for m in bad:
        add("ssdhip_ssd7_head_wgrad_workspace_bytes", m + (64, 48))
    for ci, cp in ((96, 48), (3, 48), (64, 64), (64, 32)):
        add("ssdhip_ssd7_head_wgrad_workspace_bytes", maps[1] + (ci, cp))
    add("ssdhip_ssd7_head_wgrad_plan", bad[0] + (64, 48))
    add("ssdhip_ssd7_head_wgrad_plan", maps[1] + (64, 64))
    return q


class _Env:
    def __init__(self, env):
        self.env, self.old = env or {}, {}

    def __enter__(self):
        for k, v in self.env.items():
            self.old[k] = os.environ.get(k)
            os.environ[k] = v

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def run_case(lib, entry, over, env):
    """The return code of `entry` for its base call with `over` applied."""
    args, slot, keep = [], 0, []
    for name, kind, base in ENTRIES[entry]:
        v = over.get(name, base)
        if kind == "p":
            args.append(None if v is None else _BASE + slot * _STEP + v)
            slot += 1
        elif kind == "P":
            if v is None:
                args.append(None)
            else:
                arr = (ctypes.c_void_p * len(v))(*[None if o is None else _BASE + slot * _STEP + 4096 * k + o for k, o in enumerate(v)])
                keep.append(arr)
                args.append(ctypes.cast(arr, ctypes.c_void_p))
            slot += 1
        elif kind in ("I", "L"):
            if v is None:
                args.append(None)
            else:
                args.append(((ctypes.c_int if kind == "I" else ctypes.c_longlong) * len(v))(*v))   # as void* or as a typed pointer
        else:
            args.append(v)
    with _Env(env):
        return int(getattr(lib, entry)(*args, None))


_PLAN_INTS = {"ssdhip_conv3x3_halo_plan": 4, "ssdhip_ssd7_conv_wgrad_plan": 4, "ssdhip_ssd7_head_wgrad_plan": 8}     # ints a plan query writes


def run_query(lib, name, args, env):
    with _Env(env):
        if name in _PLAN_INTS:
            plan = (ctypes.c_int * _PLAN_INTS[name])(*[-7] * _PLAN_INTS[name])
            rc = getattr(lib, name)(*args, plan)
            return [int(rc)] + list(plan)
        return int(getattr(lib, name)(*args))


def verdicts():
    lib = nat.load()
    return ({cid: run_case(lib, *c) for cid, c in cases().items()}, {qid: run_query(lib, *q) for qid, q in queries().items()})


def write_verdicts(commit):
    v, q = verdicts()
    with open(VERDICTS, "w") as f:
        json.dump({"recorded_on_commit": commit, "codes": {"accepted (no device: SSDHIP_E_LAUNCH)": -3, "SSDHIP_E_BADARG": -1,
                                                           "SSDHIP_E_WORKSPACE": -2},
                   "verdicts": v, "queries": q}, f, indent=0, sort_keys=True)
        f.write("\n")
