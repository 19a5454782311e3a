"""`build_model` (SSD7) -- drop-in for the reference builder models/keras_ssd7.py:30-430, as a torch module.

Seven conv + BatchNorm(eps 1e-3, Keras momentum 0.99) + ELU blocks with 2x2 'valid' max-pools
(:277-309); predictor heads on conv4..conv7 (:323-331).
"""
from __future__ import annotations

import copy

import numpy as np
import torch
from torch import nn
import torch.nn.functional as F

from .. import _native as nat
from ._train_fns import _AssembleTrainFn, _BnEluPoolFn, _Ssd7ConvFn, _Ssd7HeadFn
from ._common import SSDModel, he_normal_, make_priorboxes, pool_out, resolve_anchor_config


class SSD7(SSDModel):
    WIDTHS = (32, 48, 64, 64, 48, 48, 32)

    def __init__(self, image_size, n_classes, mode, l2_regularization, scales, aspect_ratios, n_boxes, steps, offsets,
                 two_boxes_for_ar1, clip_boxes, variances, coords, normalize_coords, subtract_mean, divide_by_stddev,
                 swap_channels, confidence_thresh, iou_threshold, top_k, nms_max_output_size):
        config = {k: v for k, v in locals().items() if k not in ("self", "__class__")}
        super().__init__(image_size, n_classes, mode, l2_regularization, subtract_mean, divide_by_stddev, swap_channels,
                         confidence_thresh, iou_threshold, top_k, nms_max_output_size, coords, normalize_coords)
        self._init_config = copy.deepcopy(config)         # the constructor's arguments: models/resample.py rebuilds with another n_classes
        chans = (self.img_channels,) + self.WIDTHS
        self.convs = nn.ModuleList([nn.Conv2d(chans[i], chans[i + 1], 5 if i == 0 else 3, padding=2 if i == 0 else 1)
                                    for i in range(7)])
        self.bns = nn.ModuleList([nn.BatchNorm2d(c, eps=1e-3, momentum=0.01) for c in self.WIDTHS])
        src = self.WIDTHS[3:]
        self.conf_heads = nn.ModuleList([nn.Conv2d(ch, nb * self.n_classes, 3, padding=1) for ch, nb in zip(src, n_boxes)])
        self.loc_heads = nn.ModuleList([nn.Conv2d(ch, nb * 4, 3, padding=1) for ch, nb in zip(src, n_boxes)])
        self.priorboxes = make_priorboxes(self.img_height, self.img_width, scales, aspect_ratios, two_boxes_for_ar1, steps,
                                          offsets, clip_boxes, variances, coords, normalize_coords,
                                          ['anchors4', 'anchors5', 'anchors6', 'anchors7'])
        he_normal_(self)

    def fused_blocks(self, enable=True, training=False, convolutions=False, heads=False):
        """Opt in to (or, with False, out of) running every Conv2D -> BatchNormalization -> ELU [-> MaxPooling2D] block of a bf16 model
        in eval mode under no_grad as ONE libssdhip launch (csrc/ssdhip_convbn.hip): the block's map is rounded to bf16 once instead of
        three times and is never written and read back between the convolution, the normalisation, the activation and the pool.  Off by
        default: the default bf16 path stays bit-identical to the framework's.  A model in train() mode (batch statistics) and every
        other dtype / device keep the default path whatever the switch says -- unless `training=True` asks for the training path too:
        a bf16 CUDA model in train() mode then runs what lies between a block's convolution and the next one's -- batch statistics, the
        running-statistics update, the normalisation, ELU and the pool, and their backward -- as libssdhip launches with one autograd
        node per block (csrc/ssdhip_bntrain.hip, models/_train_fns.py: _BnEluPoolFn); the convolutions stay the framework's.  A block
        whose shape those kernels do not cover keeps the default chain.
        `convolutions=True` (with `training=True`; off by default, and every call without it behaves as before) moves the seven trunk
        convolutions of that training path to libssdhip as well: one launch at the top of `features` rebuilds the packed filter images
        from the current parameters, then each block in TRAIN_CONVS runs `_Ssd7ConvFn` -- forward on the inference path's MFMA kernels
        with a bias epilogue, data gradient on the same kernels with the flipped image, weight / bias gradient in
        csrc/ssdhip_wgrad7.hip -- followed by `_BnEluPoolFn`.  The `nn.Conv2d` modules in `self.convs` are NOT called on this route
        (their parameters are read directly), so forward hooks registered on them do not fire.
        `heads=True` (with `training=True`; off by default, independent of `convolutions`, and every call without it behaves as before)
        moves what lies behind the trunk in that training path to libssdhip: one launch rebuilds the packed images and biases of the four
        source maps' heads from the current parameters, each map's conf and loc heads run as ONE 48-channel convolution under
        `_Ssd7HeadFn` (forward and data gradient on the blocks' MFMA kernels, parameter gradients in csrc/ssdhip_heads7.hip), and
        `_AssembleTrainFn` builds the prediction tensor from the four packed maps in one launch (one more backward) -- instead of
        eight framework convolutions, their permutes, reshapes, concatenations and the softmax.  All four maps or none: the route needs
        3 x 3 'same' heads with bias, bf16 weights and biases, n_boxes (n_classes + 4) <= 48 and source maps of 64, 48 or 32 channels on
        every map; anything else keeps the framework's heads.  The `nn.Conv2d` modules in `self.conf_heads` / `self.loc_heads` are NOT
        called on this route, so forward hooks registered on them do not fire.  Returns the model."""
        self.__dict__["_fused_blocks"] = bool(enable)
        self.__dict__["_fused_blocks_training"] = bool(enable) and bool(training)
        self.__dict__["_fused_blocks_convs"] = bool(enable) and bool(training) and bool(convolutions)
        self.__dict__["_fused_blocks_heads"] = bool(enable) and bool(training) and bool(heads)
        return self

    # The blocks the training path takes when it is switched on (a set, so that a measurement can take one out: DESIGN.md 4.4,
    # "SSD7 training", has the per-block numbers behind it).
    TRAIN_BLOCKS = frozenset(range(7))
    # ... and the blocks whose convolution runs in libssdhip under `convolutions=True`: those whose forward, data gradient and weight
    # gradient together beat the framework's, summed over batch 8 and 32 (same section: the per-layer timings).  Blocks 4-7 -- maps of
    # 37 x 37 and below -- do not, and keep the framework's convolution.
    TRAIN_CONVS = frozenset((0, 1, 2))

    def _fused_blocks_on(self, x):
        return (self.__dict__.get("_fused_blocks", False) and not self.training and self._fused(x)
                and self.convs[0].weight.dtype == torch.bfloat16 and self.img_channels == 3)

    def _train_blocks_on(self, x):
        return (self.__dict__.get("_fused_blocks_training", False) and self.training and x.is_cuda and x.dtype == torch.bfloat16
                and self.convs[0].weight.dtype == torch.bfloat16)

    def _train_conv_images(self):
        """{layer: (forward image, flipped image or None)} of the convolutions `convolutions=True` runs, or None when the route is off:
        the model's own buffers (allocated once per device, so a captured step keeps reading them), REWRITTEN from the current
        parameters by one launch here -- `features` calls this once per step."""
        if not self.__dict__.get("_fused_blocks_convs", False):
            return None
        dev = self.convs[0].weight.device
        hit = self.__dict__.get("_conv_images")
        if hit is None or hit[0] != dev or hit[1] != self.TRAIN_CONVS:
            layers = [i for i in sorted(self.TRAIN_CONVS)
                      if self.convs[i].bias is not None and self.convs[i].weight.dtype == self.convs[i].bias.dtype == torch.bfloat16
                      and nat.ssd7_conv_geometry(self.convs[i].in_channels, self.convs[i].out_channels, self.convs[i].kernel_size[0])]
            hit = (dev, self.TRAIN_CONVS, layers) + nat.ssd7_pack_images([self.convs[i].weight for i in layers])
            self.__dict__["_conv_images"] = hit
        _, _, layers, fwd, flipped = hit
        if not layers:
            return {}
        nat.ssd7_pack_filters([self.convs[i].weight.detach() for i in layers], fwd, flipped)
        return {i: (fwd[n], flipped[n]) for n, i in enumerate(layers)}

    def _train_block(self, i, x, images=None):
        """Block i of the training path: (the map for the next block, the map for the predictor heads or None); None where the kernels
        do not cover the block (the caller runs the default chain, which raises for a single value per channel as the framework does).
        images: `_train_conv_images()` -- a layer found there runs its convolution in libssdhip too."""
        bn = self.bns[i]
        pool, keep = i < 6, i >= 3
        b, _, h, w = x.shape
        if (i not in self.TRAIN_BLOCKS or not bn.track_running_stats or bn.momentum is None or not bn.affine
                or bn.weight.dtype != bn.bias.dtype or bn.running_mean.dtype != bn.running_var.dtype
                or nat.bn_elu_train_blocks(b * h * w, bn.num_features) == 0 or (pool and (h < 2 or w < 2))):
            return None
        conv = self.convs[i]
        image, flipped = images.get(i, (None, None)) if images else (None, None)
        if image is None or (flipped is None and x.requires_grad):
            y = conv(x)
        elif torch.is_grad_enabled():
            y = _Ssd7ConvFn.apply(x, conv.weight, conv.bias, image, flipped)
        else:
            y = nat.ssd7_conv_bias(x if x.permute(0, 2, 3, 1).is_contiguous() else x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2),
                                   image, conv.bias.detach(), conv.out_channels, conv.kernel_size[0])
        bn.num_batches_tracked.add_(1)
        args = (bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.momentum, bn.eps, pool, keep)
        if torch.is_grad_enabled():
            full, pooled = _BnEluPoolFn.apply(y, *args)[:2]
        else:
            if not y.permute(0, 2, 3, 1).is_contiguous():
                y = y.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
            full, pooled = nat.bn_elu_train_forward(y, *args)[:2]
        return (pooled if pool else full), (full if keep else None)

    def _train_heads_covered(self, feats):
        """Whether `heads=True` takes all four source maps (the conditions of `fused_blocks`' docstring, and the one-launch assembly
        backward fitting its LDS: the kernel's own formula)."""
        same = lambda c: (c.kernel_size == (3, 3) and c.stride == (1, 1) and c.padding == (1, 1) and c.dilation == (1, 1) and c.groups == 1
                          and c.bias is not None and c.weight.dtype == c.bias.dtype == torch.bfloat16 and c.weight.is_cuda)
        if not 0 < len(feats) == len(self.conf_heads) == len(self.loc_heads) <= 8:
            return False
        for f, ch, lh, pb in zip(feats, self.conf_heads, self.loc_heads, self.priorboxes):
            if not (same(ch) and same(lh) and f.is_cuda and f.dtype == torch.bfloat16 and ch.in_channels == lh.in_channels == f.shape[1]
                    and ch.out_channels == pb.n_boxes * self.n_classes and lh.out_channels == pb.n_boxes * 4
                    and nat.ssd7_head_geometry(f.shape[1], ch.out_channels, lh.out_channels)
                    and nat.ssd7_head_wgrad_plan(f.shape[0], f.shape[2], f.shape[3], f.shape[1]) is not None):
                return False
        key = (self.n_classes, tuple(int(pb.n_boxes) for pb in self.priorboxes))
        memo = self.__dict__.setdefault("_head_assembly_fits", {})
        if key not in memo:
            memo[key] = nat.assemble_backward_supported(key[0], key[1], (nat.SSD7_HEAD_CP,) * len(key[1]))
        return memo[key]

    def _model_head_route(self, feats, sizes, decode):
        """`heads=True`: the packed heads of the four source maps and the prediction assembly as libssdhip autograd nodes; None -- the
        generic head path -- when the switch is off, outside a training step under autograd, or for heads the kernels do not cover.
        The packed images and biases are the model's own buffers (allocated once per device, so a captured step keeps reading them),
        REWRITTEN from the current parameters by one launch here, once per step."""
        if (not self.__dict__.get("_fused_blocks_heads", False) or decode or not self.training or not torch.is_grad_enabled()
                or not self._train_heads_covered(feats)):
            return None
        conf_w, loc_w = [ch.weight for ch in self.conf_heads], [lh.weight for lh in self.loc_heads]
        dev = conf_w[0].device
        hit = self.__dict__.get("_head_images")
        if hit is None or hit[0] != dev:
            hit = (dev,) + nat.ssd7_head_images(conf_w, loc_w)
            self.__dict__["_head_images"] = hit
        _, fwd, flipped, bias = hit
        nat.ssd7_pack_heads([t.detach() for t in conf_w], [t.detach() for t in loc_w], [ch.bias.detach() for ch in self.conf_heads],
                            [lh.bias.detach() for lh in self.loc_heads], fwd, flipped, bias)
        ys = [_Ssd7HeadFn.apply(f, ch.weight, ch.bias, lh.weight, lh.bias, fwd[l], flipped[l], bias[l])
              for l, (f, ch, lh) in enumerate(zip(feats, self.conf_heads, self.loc_heads))]
        anchors = self.anchors_and_variances(sizes, dev)
        return _AssembleTrainFn.apply(anchors, self.n_classes, [pb.n_boxes for pb in self.priorboxes], *ys)

    def _block_sources(self, i):
        conv, bn = self.convs[i], self.bns[i]
        return (conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var)

    def _block_key(self, i):
        return tuple((t.data_ptr(), t._version) for t in self._block_sources(i))

    def _block_tables(self, i):
        """(packed filters, scale, shift) of block i for `nat.conv_bn_elu`, cached; rebuilt IN THEIR OWN STORAGE (a captured HIP graph
        keeps reading it) when the convolution's or the BatchNorm's tensors changed -- an in-place update (optimizer step,
        load_state_dict, load_keras_weights) bumps `_version`, a replaced storage changes `data_ptr()`.  The tables are computed on
        the host in float64 and rounded once: scale = gamma / sqrt(running_var + eps), shift = beta + (conv_bias - running_mean) scale."""
        cache = self.__dict__.setdefault("_block_cache", {})
        key = self._block_key(i)
        hit = cache.get(i)
        if hit is not None and hit[0] == key and hit[1].device == self.convs[i].weight.device:
            return hit[1:]
        w, b, gamma, beta, mean, var = (t.detach() for t in self._block_sources(i))
        f64 = lambda t: t.double().cpu()
        scale = f64(gamma) / torch.sqrt(f64(var) + self.bns[i].eps)
        shift = f64(beta) + (f64(b) - f64(mean)) * scale
        tables = torch.stack([scale, shift]).float().to(w.device)
        if hit is not None and hit[1].device == w.device:
            nat.conv_bn_elu_pack(w, out=hit[1])
            hit[2].copy_(tables[0])
            hit[3].copy_(tables[1])
            hit = (key,) + tuple(hit[1:])
        else:
            hit = (key, nat.conv_bn_elu_pack(w), tables[0].contiguous(), tables[1].contiguous())
        cache[i] = hit
        return hit[1:]

    def _derived_weights_key(self):
        key = super()._derived_weights_key()
        if self.__dict__.get("_block_cache"):
            key += tuple(self._block_key(i) for i in range(7))
        return key

    def _refresh_derived_weights(self):
        super()._refresh_derived_weights()
        for i in list(self.__dict__.get("_block_cache", {})):
            self._block_tables(i)

    def features(self, x):
        feats = []
        if self._fused_blocks_on(x):
            # blocks 1-3 with their pool in the launch; blocks 4-7 feed the predictor heads with their full maps, then the pooling pass
            for i in range(7):
                packed, scale, shift = self._block_tables(i)
                x = nat.conv_bn_elu(x, packed, scale, shift, 5 if i == 0 else 3, pool=i < 3)
                if i >= 3:
                    feats.append(x)
                    if i < 6:
                        x = self.max_pool(x, 2, 2)
            return feats
        train_blocks = self._train_blocks_on(x)
        images = self._train_conv_images() if train_blocks else None
        for i in range(7):
            done = self._train_block(i, x, images) if train_blocks else None
            if done is not None:
                x, feat = done
                if feat is not None:
                    feats.append(feat)
                continue
            x = F.elu(self.bns[i](self.convs[i](x)))
            if i >= 3:
                feats.append(x)
            if i < 6:
                x = self.max_pool(x, 2, 2)
        return feats

    def predictor_sizes(self):
        out = []
        for n in (self.img_height, self.img_width):
            sizes = []
            for i in range(7):
                if i >= 3:
                    sizes.append(n)
                n = pool_out(n, 2, 2)
            out.append(sizes)
        return np.array(list(zip(*out)))


def build_model(image_size, n_classes, mode='training', l2_regularization=0.0, min_scale=0.1, max_scale=0.9, scales=None,
                aspect_ratios_global=[0.5, 1.0, 2.0], aspect_ratios_per_layer=None, two_boxes_for_ar1=True, steps=None,
                offsets=None, clip_boxes=False, variances=[1.0, 1.0, 1.0, 1.0], coords='centroids', normalize_coords=False,
                subtract_mean=None, divide_by_stddev=None, swap_channels=False, confidence_thresh=0.01,
                iou_threshold=0.45, top_k=200, nms_max_output_size=400, return_predictor_sizes=False):
    '''Build the 7-layer SSD (reference keras_ssd7.py:30-54 for the arguments); see `ssd_300`.'''
    scales, ars, n_boxes, steps, offsets = resolve_anchor_config(4, min_scale, max_scale, scales, aspect_ratios_global,
                                                                 aspect_ratios_per_layer, two_boxes_for_ar1, steps,
                                                                 offsets, variances)
    model = SSD7(image_size, n_classes, mode, l2_regularization, scales, ars, n_boxes, steps, offsets, two_boxes_for_ar1,
                 clip_boxes, variances, coords, normalize_coords, subtract_mean, divide_by_stddev, swap_channels,
                 confidence_thresh, iou_threshold, top_k, nms_max_output_size)
    if return_predictor_sizes:
        return model, model.predictor_sizes()
    return model
