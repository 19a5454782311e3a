"""Shared machinery of the SSD model builders (reference models/keras_ssd300.py:200-457 and twins).

The convolutional stack of a bf16 model runs on libssdhip's MFMA kernels (csrc/ssdhip_convh / conv64 / conv /
convimg / chain .hip), dispatched here per layer shape (`SSDModel._pick` over the candidates `_conv_select` lists), with the graph glue in
csrc/ssdhip_layers.hip and, for training, the autograd functions of `_train_fns` over the same kernels (+ csrc/ssdhip_wgrad /
ssdhip_train .hip) and the bf16 weight copies of `_shadow`; the framework's own convolution (MIOpen) only runs float32 models and the few layer
geometries no kernel here covers.  Around it this module adds what the reference's graph does: in-graph input
normalisation, NHWC-ordered head reshapes so the anchor axis factorises exactly like Keras'
`Reshape((-1, n_classes))`, the resident anchor constant, softmax, the `(B, N, C+12)` prediction layout and the
optional decode layer.
"""
from __future__ import annotations

import numpy as np
import torch
from torch import nn
import torch.nn.functional as F

from .. import _native as nat
from ..anchor_math import n_boxes_for
from ..keras_layers.keras_layer_AnchorBoxes import AnchorBoxes
from ..keras_layers.keras_layer_DecodeDetections import DecodeDetections
from ..keras_layers.keras_layer_DecodeDetectionsFast import DecodeDetectionsFast
from ..keras_layers.keras_layer_L2Normalization import L2Normalization
from . import _conv_select as sel
from . import _shadow
from ._graphed import GraphedInference
from ._heads import PredictorHeads
from ._train_fns import (_AssembleTrainFn, _ConvBiasActFn, _ConvBiasActPoolFn, _MaxPoolFn, _PackedHeadFn, _ReluLink,  # noqa: F401
                         _conv_input_weight_grads)


def conv_out(n, k, s=1, p=0, d=1):
    return (n + 2 * p - d * (k - 1) - 1) // s + 1


def pool_out(n, k, s, p=0, ceil_mode=False):
    if ceil_mode:
        o = -(-(n + 2 * p - k) // s) + 1
        if (o - 1) * s >= n + p:
            o -= 1
        return o
    return (n + 2 * p - k) // s + 1


def he_normal_(module):
    for m in module.modules():
        if isinstance(m, nn.Conv2d):
            nn.init.kaiming_normal_(m.weight, mode='fan_in', nonlinearity='relu')   # Keras 'he_normal'
            if m.bias is not None:
                nn.init.zeros_(m.bias)


def resolve_anchor_config(n_predictor_layers, min_scale, max_scale, scales, aspect_ratios_global,
                          aspect_ratios_per_layer, two_boxes_for_ar1, steps, offsets, variances):
    """The argument checks and defaults of the builders (keras_ssd300.py:178-237)."""
    if aspect_ratios_global is None and aspect_ratios_per_layer is None:
        raise ValueError("`aspect_ratios_global` and `aspect_ratios_per_layer` cannot both be None. At least one needs to be specified.")
    if aspect_ratios_per_layer:
        if len(aspect_ratios_per_layer) != n_predictor_layers:
            raise ValueError("It must be either aspect_ratios_per_layer is None or len(aspect_ratios_per_layer) == {}, but "
                             "len(aspect_ratios_per_layer) == {}.".format(n_predictor_layers, len(aspect_ratios_per_layer)))
    if (min_scale is None or max_scale is None) and scales is None:
        raise ValueError("Either `min_scale` and `max_scale` or `scales` need to be specified.")
    if scales:
        if len(scales) != n_predictor_layers + 1:
            raise ValueError("It must be either scales is None or len(scales) == {}, but len(scales) == {}.".format(
                n_predictor_layers + 1, len(scales)))
    else:
        scales = np.linspace(min_scale, max_scale, n_predictor_layers + 1)
    if len(variances) != 4:
        raise ValueError("4 variance values must be pased, but {} values were received.".format(len(variances)))
    if np.any(np.array(variances) <= 0):
        raise ValueError("All variances must be >0, but the variances given are {}".format(variances))
    if (steps is not None) and (len(steps) != n_predictor_layers):
        raise ValueError("You must provide at least one step value per predictor layer.")
    if (offsets is not None) and (len(offsets) != n_predictor_layers):
        raise ValueError("You must provide at least one offset value per predictor layer.")
    ars = aspect_ratios_per_layer if aspect_ratios_per_layer else [aspect_ratios_global] * n_predictor_layers
    n_boxes = [n_boxes_for(ar, two_boxes_for_ar1) for ar in ars]
    steps = steps if steps is not None else [None] * n_predictor_layers
    offsets = offsets if offsets is not None else [None] * n_predictor_layers
    return list(scales), ars, n_boxes, steps, offsets


class SSDModel(PredictorHeads, nn.Module):
    """Base class: subclasses define `features(x) -> list of predictor feature maps` plus
    `conf_heads`, `loc_heads` (ModuleLists) and `priorboxes` (ModuleList of AnchorBoxes)."""

    def __init__(self, image_size, n_classes, mode, l2_regularization, subtract_mean, divide_by_stddev, swap_channels,
                 confidence_thresh, iou_threshold, top_k, nms_max_output_size, coords, normalize_coords):
        super().__init__()
        if mode not in ('training', 'inference', 'inference_fast'):
            raise ValueError("`mode` must be one of 'training', 'inference' or 'inference_fast', but received '{}'.".format(mode))
        self.img_height, self.img_width, self.img_channels = image_size
        self.n_classes = n_classes + 1               # incl. background, as in the reference (:175)
        self.mode = mode
        self.l2_regularization = l2_regularization
        self.subtract_mean = subtract_mean
        self.divide_by_stddev = divide_by_stddev
        self.swap_channels = swap_channels
        self.fused_inference = True         # bf16 + no_grad on a GPU: graph glue runs in libssdhip (csrc/ssdhip_layers.hip)
        self.fused_training = True          # grad mode on a GPU in bf16 (autocast): convolution forwards run in libssdhip too
        self.decoder = None
        if mode != 'training':
            layer = DecodeDetections if mode == 'inference' else DecodeDetectionsFast
            self.decoder = layer(confidence_thresh=confidence_thresh, iou_threshold=iou_threshold, top_k=top_k,
                                 nms_max_output_size=nms_max_output_size, coords=coords,
                                 normalize_coords=normalize_coords, img_height=self.img_height,
                                 img_width=self.img_width, name='decoded_predictions')
        self._anchor_cache = {}
        self._packed_heads = {}

    # -- fused inference path: every conv is followed by ONE libssdhip pass (bias + ReLU [+ max-pool]) instead of the
    #    2-3 elementwise kernels PyTorch launches; bit-identical results (see csrc/ssdhip_layers.hip) ----------------
    def _fused(self, x, conv=None):
        return (self.fused_inference and x.is_cuda and x.dtype == torch.bfloat16 and not torch.is_grad_enabled()
                and (conv is None or (conv.weight.dtype == torch.bfloat16 and conv.out_channels % 8 == 0)))

    @staticmethod
    def _conv_nobias(conv, x):
        return F.conv2d(x, conv.weight, None, conv.stride, conv.padding, conv.dilation, conv.groups)

    # Which kernel runs a convolution of the fused path: 'miopen' (F.conv2d + one libssdhip bias/ReLU[/pool] pass) or
    # 'igemm' (libssdhip's implicit-GEMM MFMA kernel with the bias/ReLU epilogue, csrc/ssdhip_conv.hip).  SSDHIP_CONV =
    # auto (default: time libssdhip's variants once per layer shape, keep the fastest), auto_miopen (MIOpen competes too),
    # igemm, miopen.
    _conv_choice = {}

    def _pick(self, key, candidates):
        """candidates: {name: thunk}; returns the name of the fastest (timed once per key with events)."""
        mode = sel.switch("CONV")
        if mode in candidates:
            return mode
        prefer = sel.switch("PREFER")              # A/B aid: this candidate wherever it is offered, the autotune elsewhere
        if prefer and prefer in candidates:
            return prefer
        if mode == "igemm" and "igemm" not in candidates:
            return "miopen"
        hit = SSDModel._conv_choice.get(key)
        if hit is None:
            if mode != "auto_miopen" and len(candidates) > 1 and "miopen" in candidates:
                # Measured on MI355X (profiles/r01*, r02b_bench.json): libssdhip's kernels beat MIOpen + one bias/ReLU pass on every
                # SSD300 / SSD512 layer, and on shapes where MIOpen has no tuned solver its find step falls back to a naive kernel
                # (~20 s of probing per process).  MIOpen is only timed when asked for (SSDHIP_CONV=auto_miopen) or when it is the
                # only candidate.
                candidates = {k: v for k, v in candidates.items() if k != "miopen"}
                if len(candidates) == 1:
                    hit = next(iter(candidates))
                    SSDModel._conv_choice[key] = hit
                    return hit
            best, hit, times = None, None, {}
            # the library candidate goes last: when MIOpen falls back to its naive solver for a shape (tens of ms per call) the
            # single-call probe below drops it without paying for the bursts
            for name in sorted(candidates, key=lambda n: n == "miopen"):
                fn = candidates[name]
                fn()
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                if best is not None:
                    a.record()
                    fn()
                    b.record()
                    b.synchronize()
                    if a.elapsed_time(b) > 3.0 * best / 4.0:
                        continue
                t = None
                for _ in range(3):                       # best of three bursts of six: one noisy burst does not decide a layer
                    a.record()
                    for _ in range(6):
                        fn()
                    b.record()
                    b.synchronize()
                    t = a.elapsed_time(b) if t is None else min(t, a.elapsed_time(b))
                times[name] = t
                if best is None or t < best:
                    best, hit = t, name
            # Near-ties go to the deeper-pipelined form: a back-to-back burst is L2-warm and host-paced, and on fc6 / conv6_1 it has put
            # the two-stage kernel a few per cent ahead of the three-stage one that is 10-25 % faster inside the step
            # (profiles/r04s_step_timeline.json against r04n: fc6 142 vs 128 us, conv6_1 28 vs 22 us).
            # (plain convolutions only: among the pooled forms "halo" is the UNFUSED slab kernel + a pooling pass.)
            # Only the two-stage kernel (or the library) loses a near-tie: a measured winner among the deeper forms stays the winner,
            # and among the deeper forms within 8 % of it the FASTEST takes over, not the first of a fixed list.
            if key and key[0] == "act" and hit in ("igemm", "miopen"):
                near = [(times[name], name) for name in ("halo", "image", "igemm6", "igemm5")  # fc6 in the step: igemm6 128 us, igemm 142, igemm5 ~165 (r04n / r04s / r04zz)
                        if name in times and times[name] <= 1.08 * best]
                if near:
                    hit = min(near)[1]
            SSDModel._conv_choice[key] = hit
        return hit

    @staticmethod
    def _gemm_1x1(conv, x, relu):
        b, c, h, w = x.shape
        x2 = x.permute(0, 2, 3, 1).reshape(b * h * w, c)                 # a view of channels_last memory
        w2 = conv.weight.reshape(conv.out_channels, c)
        y2 = (torch._addmm_activation(conv.bias, x2, w2.t(), use_gelu=False) if relu else torch.addmm(conv.bias, x2, w2.t()))
        return y2.view(b, h, w, conv.out_channels).permute(0, 3, 1, 2)

    def conv_act(self, conv, x, relu=True, link_in=None, link_out=None):
        """Conv2D(activation='relu' | None).  link_in / link_out (_ReluLink, training step only; see `relu_link`): x is the ReLU output of a
        layer that feeds nothing but this one / this layer's output feeds exactly one layer, which holds the same link as its link_in."""
        if link_out is not None and not relu:
            raise ValueError("link_out on a layer without ReLU: its consumer would mask the data gradient by an activation that has no threshold")
        if self._fused(x, conv):
            g = sel.geometry_of(conv, x)
            if sel.first_layer(g):
                return nat.conv3x3_cin3(x, conv.weight, conv.bias, relu=relu)
            cands = {"miopen": lambda: nat.bias_act(self._conv_nobias(conv, x), conv.bias, relu=relu)}
            for name, fn in sel.candidates(g, relu, sel.INFERENCE).items():
                cands[name] = lambda fn=fn: fn(x, conv.weight, conv.bias)
            if sel.igemm(g) and g.k == 1 and sel.on("GEMM_1X1"):
                # a 1 x 1 layer on NHWC memory IS a plain GEMM ([B H W, Cin] x [Cin, Cout] + bias, ReLU).  Opt-in: the library's
                # (hipBLASLt through torch, bias / activation in its epilogue) was measured on fc7 and conv6_1 inside the step and is
                # no faster than the implicit-GEMM kernels (profiles/r05zd_library_gemm_for_1x1_layers_ab.txt: 2.119 / 2.112 / 2.119 ms)
                cands["gemm"] = lambda: self._gemm_1x1(conv, x, relu)
            if len(cands) == 1:
                return cands["miopen"]()
            name = sel.untimed_choice(g, relu) or self._pick(sel.act_key(g, relu), cands)
            return cands[name]()
        if self._fused_train(x, conv):
            run, _name = self._train_thunk(conv, x, relu)
            if run is not None:
                wb, bb, wt = self._bf16_shadow(conv, with_transposed=True)
                return _ConvBiasActFn.apply(x, conv.weight, conv.bias, run, conv.stride, conv.padding, conv.dilation, relu, wb, bb, wt,
                                            link_in, link_out)
        y = conv(x)
        return F.relu(y) if relu else y

    # -- training step: the forward of every convolution libssdhip has a kernel for runs there (under autograd, see
    #    _ConvBiasActFn); pooling stays a separate PyTorch op because its backward needs the pre-pool activation ---------------
    def _fused_train(self, x, conv):
        return (self.fused_training and x.is_cuda and torch.is_grad_enabled() and conv.bias is not None and conv.groups == 1
                and (x.dtype == torch.bfloat16 or (torch.is_autocast_enabled() and torch.get_autocast_dtype("cuda") == torch.bfloat16)))

    def _bf16_shadow(self, conv, with_transposed=False):
        """bf16 copies of a convolution's float32 master weight (channels_last) and bias for the libssdhip kernels [+ the transposed,
        tap-flipped filters of its data gradient, or None]; (None, None[, None]) for a convolution the shadow set does not hold."""
        if conv.weight.dtype == torch.bfloat16:
            return (conv.weight.detach(), conv.bias.detach(), None) if with_transposed else (conv.weight.detach(), conv.bias.detach())
        st = _shadow.fresh(self, conv.weight.device)
        i = st.index.get(id(conv))
        if i is None:
            return (None, None, None) if with_transposed else (None, None)
        if with_transposed:
            packed = st.tr_arg[i][0] != conv.out_channels                  # a head's rows live in its source map's packed tensor
            return st.cl[i], st.bias[i], (None if packed else st.tr[i])
        return st.cl[i], st.bias[i]

    def _packed_head_shadow(self, l):
        """(packed filters (Cp, Cin, 3, 3) bf16 channels_last, packed bias (Cp,), transposed / flipped (Cin, Cp, 3, 3), n_conf, n_loc) of
        predictor layer l, up to date; None when the heads of that source map are not packed."""
        ch = self.conf_heads[l]
        if ch.weight.dtype == torch.bfloat16:
            return None
        return _shadow.fresh(self, ch.weight.device).packs.get(l)

    def _train_thunk(self, conv, x, relu):
        """The libssdhip kernel for this layer as `(x_bf16, w_bf16, b_bf16) -> y`, or (None, None).  The variant is the one the
        per-shape autotune keeps (same keys as the inference path)."""
        g = sel.geometry_of(conv, x)
        if sel.first_layer(g):
            return (lambda xb, wb, bb: nat.conv3x3_cin3(xb, wb, bb, relu=relu)), "cin3"
        cands = sel.candidates(g, relu, sel.TRAINING)
        if not cands:
            return None, None
        key = sel.act_key(g, relu)
        forced = sel.switch("CONV")
        if len(cands) == 1:
            name = "igemm"
        elif forced in cands:
            name = forced
        elif SSDModel._conv_choice.get(key) in cands:
            name = SSDModel._conv_choice[key]                   # settled earlier: no bf16 copies of x / weight / bias just to look it up
        else:
            with torch.no_grad():
                xb = x.detach().to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
                wb = conv.weight.detach().to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
                bb = conv.bias.detach().to(torch.bfloat16)
                name = self._pick(key, {n: (lambda fn=fn: fn(xb, wb, bb)) for n, fn in cands.items()})
            if name not in cands:
                name = "igemm"
        return cands[name], name

    @staticmethod
    def relu_link():
        """A link between two consecutive ReLU convolutions of the training step (the lower one's output feeds ONLY the upper one): pass it
        as `link_out` of the lower layer's conv_act and `link_in` of the upper layer's conv_act / conv_act_pool.  None outside autograd -- the
        inference paths take no links.  Gradients observed at a linked intermediate activation (hooks, `retain_grad`) are already masked by the layer below."""
        return _ReluLink() if torch.is_grad_enabled() else None

    def conv_act_pool(self, conv, x, kernel, stride, pad=0, ceil_mode=False, link_in=None):
        if self._fused(x, conv):
            cands = {"miopen": lambda: nat.bias_act_maxpool(self._conv_nobias(conv, x), conv.bias, kernel, stride, pad, ceil_mode,
                                                            relu=True)}
            for name, fn in sel.pooled_candidates(sel.geometry_of(conv, x), kernel, stride, pad, ceil_mode).items():
                cands[name] = lambda fn=fn: fn(x, conv.weight, conv.bias)
            name = (self._pick(("pool", tuple(x.shape), conv.out_channels, conv.kernel_size[0], conv.dilation[0], kernel, stride, pad),
                               cands) if len(cands) > 1 else "miopen")
            return cands[name]()
        if kernel == 2 and stride == 2 and pad == 0 and ceil_mode and self._fused_train(x, conv) and sel.pool_bwd_fused(sel.geometry_of(conv, x)):
            run, _name = self._train_thunk(conv, x, True)
            if run is not None:
                wb, bb, wt = self._bf16_shadow(conv, with_transposed=True)
                return _ConvBiasActPoolFn.apply(x, conv.weight, conv.bias, run, conv.stride, conv.padding, conv.dilation, wb, bb, wt, link_in)
        return self.max_pool(self.conv_act(conv, x, relu=True, link_in=link_in), kernel, stride, pad, ceil_mode=ceil_mode)

    def conv1_block_pool(self, c1, c2, x):
        """conv1_1 -> conv1_2 -> MaxPooling2D(2, 2, 'same') (models/keras_ssd300.py:274-276).  On the fused bf16 inference path the
        three can run as ONE kernel that never writes the 64-channel full-resolution map (csrc/ssdhip_conv64.hip, FRONT); timed once
        per shape against the two-kernel form."""
        if (sel.switch("CONV") in ("auto", "auto_miopen") and self._fused(x, c1) and self._fused(x, c2)
                and sel.conv1_block(sel.geometry_of(c1), sel.geometry_of(c2))):
            cands = {"separate": lambda: self.conv_act_pool(c2, self.conv_act(c1, x), 2, 2, ceil_mode=True),
                     "conv1_block": lambda: nat.conv1_block(x, c1.weight, c1.bias, c2.weight, c2.bias, relu=True, pool=True)}
            key = ("conv1_block", tuple(x.shape), c2.out_channels)
            if SSDModel._conv_choice.get(key) is None:
                cands["separate"]()                          # settles the inner per-layer choices before the two forms are compared
            name = self._pick(key, cands)
            return cands[name if name in cands else "separate"]()       # a forced SSDHIP_CONV mode names per-layer kernels: two-kernel form
        return self.conv_act_pool(c2, self.conv_act(c1, x), 2, 2, ceil_mode=True)

    def max_pool(self, x, kernel, stride, pad=0, ceil_mode=False):
        if self._fused(x) and x.shape[1] % 8 == 0:
            return nat.bias_act_maxpool(x, None, kernel, stride, pad, ceil_mode, relu=False)
        if (self.fused_training and x.is_cuda and x.dtype == torch.bfloat16 and torch.is_grad_enabled() and x.shape[1] % 8 == 0
                and x.requires_grad and not sel.on("NO_OWN_POOL")):
            return _MaxPoolFn.apply(x, kernel, stride, pad, ceil_mode)
        return F.max_pool2d(x, kernel, stride, pad, ceil_mode=ceil_mode)

    # -- in-graph input pipeline (keras_ssd300.py:247-272): NHWC 0..255 -> normalised NCHW (channels_last memory) --
    def preprocess(self, images):
        x = images
        if x.dim() != 4:
            raise ValueError("expected images of shape (batch, height, width, channels)")
        nhwc = x.shape[-1] == self.img_channels and x.shape[1] != self.img_channels
        if (nhwc and self.fused_inference and x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()
                and not torch.is_grad_enabled() and self.img_channels <= 4
                and next(self.parameters()).dtype == torch.bfloat16):
            return nat.preprocess(x, self.subtract_mean, self.divide_by_stddev,
                                  list(self.swap_channels) if self.swap_channels else None)
        if (nhwc and self.fused_training and x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and torch.is_grad_enabled()
                and not x.requires_grad and self.img_channels <= 4 and torch.is_autocast_enabled()
                and torch.get_autocast_dtype("cuda") == torch.bfloat16 and not sel.on("NO_TRAIN_PREPROCESS")):
            # the training step under bf16 autocast: the first convolution casts its input to bf16 anyway, and the images need no
            # gradient -- the same one-launch kernel instead of a subtraction, an index_select and two layout / dtype copies
            return nat.preprocess(x, self.subtract_mean, self.divide_by_stddev,
                                  list(self.swap_channels) if self.swap_channels else None)
        if nhwc:
            x = x.permute(0, 3, 1, 2)                # NHWC storage == channels_last NCHW: no copy
        x = x.float()
        # the per-channel constants live on the device (built once): nothing crosses PCIe per call, and the step can be captured
        # into a HIP graph (a host -> device copy is not allowed while a stream is capturing)
        if self.subtract_mean is not None:
            x = x - self._device_const("mean", x.device, lambda: torch.as_tensor(self.subtract_mean, dtype=torch.float32).view(1, -1, 1, 1))
        if self.divide_by_stddev is not None:
            x = x / self._device_const("std", x.device, lambda: torch.as_tensor(self.divide_by_stddev, dtype=torch.float32).view(1, -1, 1, 1))
        if self.swap_channels:
            x = x.index_select(1, self._device_const("swap", x.device, lambda: torch.as_tensor(list(self.swap_channels), dtype=torch.long)))
        return x.contiguous(memory_format=torch.channels_last)

    def _device_const(self, name, device, build):
        key = ("const", name, str(device))
        t = self._anchor_cache.get(key)
        if t is None:
            t = build().to(device)
            self._anchor_cache[key] = t
        return t

    def anchors_and_variances(self, feature_sizes, device):
        """(N, 8) float32 constant, resident per device."""
        key = (tuple(feature_sizes), str(device))
        t = self._anchor_cache.get(key)
        if t is None:
            t = torch.cat([pb.constant(h, w, device).reshape(-1, 8) for pb, (h, w) in zip(self.priorboxes, feature_sizes)], dim=0)
            self._anchor_cache[key] = t
        return t

    def predictor_sizes(self):
        raise NotImplementedError

    def precise(self, enable=True, check_finite=True):
        """Make the REFERENCE's precision on the MFMA path this model's forward path (models/precise.py: float32 weights, every
        activation and filter a float16 (hi, lo) pair, three float16 MFMA products per multiplication, float32 accumulation; per-layer
        power-of-two range scales with an overflow guard): `model(images)` / `model.raw_predictions(images)` of a float32 CUDA model
        under no_grad then run there -- 2.6 x the framework's float32 convolutions at batch 32, predictions within ~1e-6 of them.
        `model.precise(False)` switches back.  Returns the model.  Reference: models/keras_ssd300.py:274-419 (a float32 graph)."""
        if not enable:
            self.__dict__["_precise"] = None
            return self
        from .precise import PreciseForward
        self.__dict__["_precise"] = PreciseForward(self, check_finite=check_finite)
        return self

    def raw_predictions(self, images, decode=False):
        """The `(batch, #boxes, #classes + 12)` prediction tensor; with `decode=True` (used by `forward` in the inference modes) the
        decoded detections, which on the fused bf16 path come straight from the head outputs."""
        pf = self.__dict__.get("_precise")
        if (pf is not None and images.is_cuda and not torch.is_grad_enabled() and next(self.parameters()).dtype == torch.float32):
            return pf(images, decode=bool(decode and self.decoder is not None))
        self.__dict__["_shadow_fresh"] = False
        self.__dict__["_in_forward"] = True
        try:
            return self._raw_predictions(images, decode)
        finally:
            self.__dict__["_in_forward"] = False

    def _raw_predictions(self, images, decode):
        x = self.preprocess(images)
        dtype = next(self.parameters()).dtype
        xin = x.to(dtype) if not torch.is_autocast_enabled() else x
        split = self._split_heads(xin)
        if split is not None:
            feats, confs = split
            sizes = [(f.shape[2], f.shape[3]) for f in feats]
            anchors = self.anchors_and_variances(sizes, x.device)
            head_args = (confs, [None] * len(confs), [ch.bias for ch in self.conf_heads], [lh.bias for lh in self.loc_heads],
                         [pb.n_boxes for pb in self.priorboxes], anchors, self.n_classes)
            if decode and self.decoder is not None and self.n_classes <= 81:
                return self.decoder.forward_from_heads(*head_args)
            pred = nat.assemble_predictions(*head_args)
            return self.decoder(pred) if (decode and self.decoder is not None) else pred
        feats = self.features(xin)
        b = x.shape[0]
        sizes = [(f.shape[2], f.shape[3]) for f in feats]
        own = self._model_head_route(feats, sizes, decode)
        if own is not None:
            return own
        if all(self._fused_head_ok(f, ch) for f, ch in zip(feats, self.conf_heads)):
            # heads without bias; bias, Reshape, softmax, anchors and the concatenations are one libssdhip pass (:363-419)
            packable = all(self._packed_head_ok(ch, lh, f) for f, ch, lh in zip(feats, self.conf_heads, self.loc_heads))
            how = "per_layer"
            if packable and len(feats) <= 8:
                # all packed heads as ONE grouped launch vs one launch per layer: the 1x1..5x5 heads are single workgroups
                # walking long K loops (pure latency); side by side they hide behind the 38x38 / 19x19 heads
                hc = {"per_layer": lambda: self._heads_per_layer(feats), "grouped": lambda: self._heads_grouped(feats)}
                if self._halo_heads_ok(feats):
                    hc["halo_grouped"] = lambda: self._heads_halo_grouped(feats)
                elif self._halo_heads_mixed_ok(feats):
                    hc["halo_mixed"] = lambda: self._heads_halo_mixed(feats)
                how = self._pick(("heads", tuple(tuple(f.shape) for f in feats), self.n_classes), hc)
            confs, locs = (self._heads_halo_grouped(feats) if how == "halo_grouped" else
                           self._heads_halo_mixed(feats) if how == "halo_mixed" else
                           self._heads_grouped(feats) if how == "grouped" else self._heads_per_layer(feats))
            anchors = self.anchors_and_variances(sizes, x.device)
            head_args = (confs, locs, [ch.bias for ch in self.conf_heads], [lh.bias for lh in self.loc_heads],
                         [pb.n_boxes for pb in self.priorboxes], anchors, self.n_classes)
            if decode and self.decoder is not None and self.n_classes <= 81:
                return self.decoder.forward_from_heads(*head_args)          # y_pred is never materialised
            pred = nat.assemble_predictions(*head_args)
            return self.decoder(pred) if (decode and self.decoder is not None) else pred
        if (torch.is_grad_enabled() and not decode and not sel.on("NO_TRAIN_ASSEMBLY") and len(feats) <= 8
                and all(self._packed_train_head_ok(f, ch, lh) for f, ch, lh in zip(feats, self.conf_heads, self.loc_heads))
                and self._train_assembly_fits(len(feats))):
            # every source map's heads are one packed libssdhip node: the assembly and its backward are one launch each (the backward
            # kernel stages two 128-anchor row tiles + a packed stage in LDS; whether that fits is the kernel's own formula,
            # nat.assemble_backward_supported -- 21 classes need 36 KB, COCO's 81 classes 117 KB of the CU's 160)
            ys = []
            for l, (f, ch, lh) in enumerate(zip(feats, self.conf_heads, self.loc_heads)):
                pw, pb, pwt, _nc, _nl = self._packed_head_shadow(l)
                ys.append(_PackedHeadFn.apply(f, ch.weight, ch.bias, lh.weight, lh.bias, pw, pb, pwt))
            anchors = self.anchors_and_variances(sizes, x.device)
            return _AssembleTrainFn.apply(anchors, self.n_classes, [pb_.n_boxes for pb_ in self.priorboxes], *ys)
        confs, locs = [], []
        for f, ch, lh in zip(feats, self.conf_heads, self.loc_heads):
            # NCHW -> NHWC before the reshape so the channel axis splits as (box, class) like Keras (:363-383)
            if self._packed_train_head_ok(f, ch, lh):
                pw, pb, pwt, _nc, _nl = self._packed_head_shadow(len(confs))
                y = _PackedHeadFn.apply(f, ch.weight, ch.bias, lh.weight, lh.bias, pw, pb, pwt).permute(0, 2, 3, 1)
                confs.append(y[..., :ch.out_channels].reshape(b, -1, self.n_classes))
                locs.append(y[..., ch.out_channels:ch.out_channels + lh.out_channels].reshape(b, -1, 4))
                continue
            confs.append(ch(f).permute(0, 2, 3, 1).reshape(b, -1, self.n_classes))
            locs.append(lh(f).permute(0, 2, 3, 1).reshape(b, -1, 4))
        conf = torch.softmax(torch.cat(confs, dim=1).float(), dim=-1)          # 'mbox_conf_softmax' (:415)
        loc = torch.cat(locs, dim=1).float()
        anchors = self.anchors_and_variances(sizes, conf.device)
        pred = torch.cat([conf, loc, anchors.unsqueeze(0).expand(b, -1, -1)], dim=2)   # 'predictions' (:419)
        return self.decoder(pred) if (decode and self.decoder is not None) else pred

    def _model_head_route(self, feats, sizes, decode):
        """A model's own way from the source maps to the predictions, tried ahead of the generic head paths: the prediction tensor, or
        None -- always, here -- for "take the generic path" (SSD7 overrides it for `fused_blocks(..., heads=True)`)."""
        return None

    def _derived_weights_key(self):
        """Versions of every parameter some cached, derived tensor was built from (what a captured graph cannot follow by itself)."""
        gammas = tuple((m.gamma.data_ptr(), m.gamma._version) for m in self.modules()
                       if isinstance(m, L2Normalization) and m.gamma is not None)
        return self._head_weights_key() + gammas

    def _refresh_derived_weights(self):
        self._refresh_packed_heads()
        for m in self.modules():
            if isinstance(m, L2Normalization):
                m.refresh_cached_gamma()

    def _fused_head_ok(self, f, conv):
        return (self.fused_inference and f.is_cuda and f.dtype == torch.bfloat16 and not torch.is_grad_enabled()
                and conv.weight.dtype == torch.bfloat16)

    def forward(self, images):
        return self.raw_predictions(images, decode=self.decoder is not None)

    def head_outputs(self, images):
        """The convolution stack alone: the in-graph input pipeline, every trunk / extra layer and the packed predictor heads -- what
        `forward` runs in front of DecodeDetections (or of the prediction assembly), nothing behind it.  Returns the list of packed
        head maps (one per source map, conf | loc channels).  bench.py times a HIP graph of it for `conv_roofline.forward_ms`."""
        if torch.is_grad_enabled():
            raise RuntimeError("head_outputs is an inference-path probe: call it under torch.no_grad()")
        self.__dict__["_shadow_fresh"] = False
        self.__dict__["_in_forward"] = True
        had = self.__dict__.get("_head_overlap")
        if not had:
            self.__dict__["_head_overlap"] = "4"           # outside a graph capture too: the graph step's two-stream schedule
        try:
            x = self.preprocess(images)
            split = self._split_heads(x.to(next(self.parameters()).dtype))
            if split is None:
                raise RuntimeError("head_outputs: this model / input does not take the fused inference path")
            return list(split[1])
        finally:
            self.__dict__["_head_overlap"] = had
            self.__dict__["_in_forward"] = False

    def graphed(self, images, warmup=3, heads_only=False):
        """`forward` for inputs of this shape captured ONCE into a HIP graph: a step is then a single graph launch instead of ~45
        kernel launches issued from Python (the step is 3 ms of GPU work; on a slow or busy host the eager launches alone can take
        longer).  Returns a callable; see GraphedInference.  `heads_only`: the graph of `head_outputs` (the convolution stack with the
        same two-stream schedule, no decode)."""
        return GraphedInference(self, images, warmup, fn=self.head_outputs if heads_only else None)

    predict = forward

    def l2_regularization_loss(self):
        """Keras adds l2(l2_reg) * sum(W^2) over every conv kernel (not biases) to the loss (:274 kernel_regularizer)."""
        if not self.l2_regularization:
            return torch.zeros((), device=next(self.parameters()).device)
        return self.l2_regularization * sum((m.weight.float() ** 2).sum() for m in self.modules() if isinstance(m, nn.Conv2d))


def make_priorboxes(img_height, img_width, scales, aspect_ratios, two_boxes_for_ar1, steps, offsets, clip_boxes,
                    variances, coords, normalize_coords, names):
    return nn.ModuleList([
        AnchorBoxes(img_height, img_width, this_scale=scales[i], next_scale=scales[i + 1], aspect_ratios=aspect_ratios[i],
                    two_boxes_for_ar1=two_boxes_for_ar1, this_steps=steps[i], this_offsets=offsets[i],
                    clip_boxes=clip_boxes, variances=variances, coords=coords, normalize_coords=normalize_coords,
                    name=names[i])
        for i in range(len(names))])
