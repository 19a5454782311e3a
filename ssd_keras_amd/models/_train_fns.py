"""The training step's autograd functions over the libssdhip kernels (csrc/ssdhip_train.hip, ssdhip_wgrad.hip and the forward
kernels of the inference path): one node per convolution layer [+ pooling], per pair of predictor heads, for the prediction assembly,
for a max-pool, for what follows a convolution in a block of SSD7 (batch-statistics BatchNorm + ELU [+ pool],
csrc/ssdhip_bntrain.hip), for that convolution itself (csrc/ssdhip_convbn.hip, ssdhip_wgrad7.hip) and for the pair of predictor heads
of one of SSD7's source maps (csrc/ssdhip_heads7.hip).  `SSDModel` (models/_common.py) applies them; which kernel runs a layer's forward [+ pool]
and its gradients is `_conv_select`'s choice: the convolution nodes here only map the names it returns to `_native` calls."""
import torch

from .. import _native as nat
from . import _conv_select as sel


class _ReluLink:
    """Training step, two ReLU convolutions in a row where the upper one is the lower one's ONLY consumer (conv2_1 -> conv2_2, conv3_1 ->
    conv3_2 -> conv3_3, conv4_1 -> conv4_2 -> conv4_3): the upper layer's data gradient can leave its kernel already masked by its
    input > 0 -- which is the lower layer's threshold_backward -- so the lower layer skips its pass over (dL/dy, y).  The link is how the
    two autograd nodes agree: the upper node's backward sets `masked` only when its kernel really applied the mask, the lower node's
    backward (which autograd runs after it) consumes the flag and falls back to its own mask otherwise."""
    __slots__ = ("masked", "partial")

    def __init__(self):
        self.masked = False
        self.partial = None      # the masked gradient's channel sums by workgroup ([rows, C] float32): the lower layer's bias-gradient partials


# -- what the two convolution nodes share; their ctx.conf is (stride, padding, dilation, ..., dtype of weight, of bias | None, of x) --------
def _bf16_operands(x, weight, bias, wb, bb):
    """Forward prologue: x as a bf16 NHWC map; the shadow set's bf16 filters and bias (wb, bb), cast here where there is none at hand."""
    xb = x.detach().to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    if wb is None:
        wb = weight.detach().to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        bb = bias.detach().to(torch.bfloat16) if bias is not None else None
    return xb, wb, bb


def _node_result(ctx, gx, gw, gb):
    """The gradients in the dtypes of x, weight and bias (needs_input_grad[2] is False where bias is None), None for the forward's other arguments."""
    wdt, bdt, xdt = ctx.conf[-3:]
    grads = (gx.to(xdt) if gx is not None else None), gw.to(wdt), (gb.to(bdt) if ctx.needs_input_grad[2] else None)
    return grads + (None,) * (len(ctx.needs_input_grad) - 3)


def _node_backward(ctx, gy, partial, link_in):
    """Backward epilogue, from the masked dL/dy and the per-workgroup partials of its channel sums (or None), which make the bias gradient."""
    xb, wb, _y, wt = ctx.saved_tensors
    want_gb = ctx.needs_input_grad[2]
    gx, gw, gb = _conv_input_weight_grads(gy, xb, wb, *ctx.conf[:3], ctx.needs_input_grad[0], wt, partial if want_gb else None, link_in)
    if want_gb and gb is None:
        gb = nat.row_sums(partial) if partial is not None else gy.sum(dim=(0, 2, 3), dtype=torch.float32)
    return _node_result(ctx, gx, gw, gb)


class _ConvBiasActFn(torch.autograd.Function):
    """A convolution layer of the TRAINING step with libssdhip's MFMA kernel in the forward pass (convolution + bias + ReLU, one
    kernel, bf16 NHWC -- the same kernels the inference path runs) and libssdhip's data / weight gradients behind it
    (`_conv_input_weight_grads`: since round 6 every layer of SSD300 / SSD512 except a 4 x 4 or grouped convolution, which fall to the
    framework's convolution_backward).  `run` is the libssdhip thunk picked for this layer shape: (x_bf16, w_bf16, b_bf16) -> y."""

    @staticmethod
    def forward(ctx, x, weight, bias, run, stride, padding, dilation, relu, wb=None, bb=None, wt=None, link_in=None, link_out=None):
        xb, wb, bb = _bf16_operands(x, weight, bias, wb, bb)
        y = run(xb, wb, bb)
        # (wt: the data gradient's filters, built with the shadows -- None: built in backward; saved like the others so that autograd's
        #  version check covers it when the shadows are refreshed between this forward and its backward)
        ctx.save_for_backward(xb, wb, y if relu else None, wt)
        ctx.conf = (stride, padding, dilation, relu, weight.dtype, None if bias is None else bias.dtype, x.dtype)
        # link_in: x is the ReLU output of a layer that feeds nothing else (_ReluLink); link_out: the same towards this layer's consumer
        ctx.links = (link_in, link_out if relu else None)
        return y

    @staticmethod
    def backward(ctx, gy):
        xb, wb, y, _wt = ctx.saved_tensors
        relu = ctx.conf[3]
        gy = gy.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        if sel.first_layer_bwd(sel.geometry_of_grads(wb, xb, *ctx.conf[:3]), relu, ctx.needs_input_grad[0], gy.is_cuda):
            return _node_result(ctx, None, *nat.conv1_1_backward(gy, y, xb))
        link_in, link_out = ctx.links
        premasked, partial = False, None
        if relu and link_out is not None:                # consumed here: the consumer's next backward sets them again
            premasked, partial = link_out.masked, link_out.partial
            link_out.masked, link_out.partial = False, None
        if premasked:
            # dL/dy arrived masked by y > 0 from the consumer's data-gradient kernel (_ReluLink), its channel sums beside it
            if partial is None and ctx.needs_input_grad[2]:
                partial = nat.channel_sums_partial(gy)
        elif relu:
            # ReLU mask and the per-workgroup channel sums of the bias gradient in ONE libssdhip pass (csrc/ssdhip_train.hip)
            fused = nat.relu_bwd_bias(gy, y, reduce=False)
            gy, partial = fused if fused is not None else (torch.ops.aten.threshold_backward(gy, y, 0), partial)
        return _node_backward(ctx, gy, partial, link_in)


# `_conv_select.WGRAD_FORMS` as launches: None (the kernel declines), dw, or (dw, db) when the bias partials ride in its reduction launch
_WGRAD_LAUNCH = {
    "grid": lambda g, xb, gy, partial: nat.conv3x3_wgrad(xb, gy, bias_partial=partial),
    "pixels": lambda g, xb, gy, partial: nat.conv1x1_wgrad(xb, gy, bias_partial=partial),
    "taps": lambda g, xb, gy, partial: nat.conv3x3_taps_wgrad(xb, gy, g.stride, g.padding, g.dilation, bias_partial=partial),
}


def _conv_input_weight_grads(gy, xb, wb, stride, padding, dilation, need_x, wt=None, bias_partial=None, link_in=None):
    """dL/dx, dL/dw [and dL/db] of a convolution from the (masked) dL/dy, on the kernels `_conv_select` names (`dgrad`, `wgrad_forms`).
    Data gradient: a stride-1 'same' layer through the forward's MFMA kernels on the transposed, tap-flipped filters; a strided or
    'valid' 3 x 3 layer the same way behind an embedding launch (round 6).  What no kernel covers (3 input channels, predictor heads
    whose channel counts are not multiples of 64) goes to aten.convolution_backward (MIOpen).
    bias_partial: per-workgroup channel sums of gy ([rows, Cout] float32); the third result is their ordered sum when the weight
    gradient's reduction launch could add them on the side, None otherwise (the caller reduces them itself).  link_in (_ReluLink) is
    set where the slab kernel wrote dL/dx masked by xb > 0 (the layer below then skips its own mask pass)."""
    gx = None
    g = sel.geometry_of_grads(wb, xb, stride, padding, dilation)
    form, run, masked = sel.dgrad(g, gy.is_cuda, link_in is not None and gy.dtype == xb.dtype == torch.bfloat16) if need_x else (None,) * 3
    if form:
        gz = gy if form == "same" else nat.embed_strided(gy, xb.shape[2], xb.shape[3], stride[0], 1 - padding[0])
        if wt is None:                                   # (the shadow set hands the transposed filters over: csrc/ssdhip_optim.hip)
            wt = wb.flip(2, 3).permute(1, 0, 2, 3).contiguous(memory_format=torch.channels_last)
        got = nat.conv3x3_halo_masked(gz, wt, xb, sums=masked == "sums") if masked else None
        if got is not None:
            gx, link_in.partial = got if isinstance(got, tuple) else (got, None)
            link_in.masked = True
        else:
            gx = run(gz, wt, None)
    launches = (_WGRAD_LAUNCH[name](g, xb, gy, bias_partial) for name in sel.wgrad_forms(g, gy.is_cuda))
    gw = next((got for got in launches if got is not None), None)          # the first form that does not decline
    gw, gb = gw if (gw is not None and bias_partial is not None) else (gw, None)
    masks = [need_x and gx is None, gw is None, False]
    if masks[0] or masks[1]:
        gx_m, gw_m, _ = torch.ops.aten.convolution_backward(gy, xb, wb, None, list(stride), list(padding), list(dilation), False, [0, 0],
                                                            1, masks)
        gx, gw = (gx_m if masks[0] else gx), (gw_m if masks[1] else gw)
    return gx, gw, gb


class _ConvBiasActPoolFn(torch.autograd.Function):
    """Conv2D(relu) -> MaxPooling2D(2, 2, 'same') of the TRAINING step (pool1 .. pool3) as one autograd node: forward = ONE launch that
    writes both maps where `_conv_select.pool_keep` has a form for the layer (round 6), the layer's MFMA kernel + the one-pass pooling
    kernel otherwise; backward = max-pool gradient, ReLU mask and bias gradient in ONE pass over the full-resolution map (csrc/
    ssdhip_train.hip, maxpool2_relu_bwd_bias_kernel: the unmasked gradient is never written), then the convolution's as in _ConvBiasActFn."""

    @staticmethod
    def forward(ctx, x, weight, bias, run, stride, padding, dilation, wb=None, bb=None, wt=None, link_in=None):
        xb, wb, bb = _bf16_operands(x, weight, bias, wb, bb)
        ctx.link_in = link_in
        keep = sel.pool_keep(sel.geometry_of_grads(wb, xb, stride, padding, dilation), xb.is_cuda)
        kept = {"c64": nat.conv3x3_c64_pool_keep, "halo": nat.conv3x3_halo_pool_keep}[keep](xb, wb, bb, relu=True) if keep else None
        if kept is None:                                 # (no such form for the layer, or the slab kernel declines)
            y = run(xb, wb, bb)
            kept = y, nat.bias_act_maxpool(y, None, 2, 2, 0, True, relu=False)
        y, p = kept
        ctx.save_for_backward(xb, wb, y, wt)
        ctx.conf = (stride, padding, dilation, weight.dtype, None if bias is None else bias.dtype, x.dtype)
        return p

    @staticmethod
    def backward(ctx, gp):
        gp = gp.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        fused = nat.maxpool2_relu_bwd_bias(ctx.saved_tensors[2], gp, reduce=False)
        if fused is None:
            raise RuntimeError("channel count not supported by the fused pooling backward (the forward checks it)")
        return _node_backward(ctx, *fused, ctx.link_in)


class _PackedHeadFn(torch.autograd.Function):
    """The two predictor heads of one source map in the TRAINING step as one libssdhip node (round 4): conf and loc filters packed along
    Cout (zero rows up to a multiple of 128), forward = the slab kernel (no activation), data gradient = the slab kernel on the flipped /
    transposed pack, weight gradient = ssdhip_conv3x3_wgrad on the packed gradient, bias gradient = one reduction -- instead of two
    framework convolutions forward and four backward per map (MIOpen: 1.7 ms of a 12.7 ms step, profiles/r04za).  Returns the packed
    (B, Cp, H, W) bf16 map; the caller slices conf / loc out of it (reference: models/keras_ssd300.py:322-335)."""

    @staticmethod
    def forward(ctx, x, wc, bc, wl, bl, pw, pb, pwt):
        """pw / pb / pwt: the packed bf16 filters [conf | loc | zero rows], biases and transposed / flipped filters of this source map,
        kept up to date with the parameters by the model's shadow set (SSDModel._packed_head_shadow): nothing is concatenated here."""
        xb = x.detach().to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        y = nat.conv3x3_halo(xb, pw, pb, relu=False, pool=False)
        ctx.save_for_backward(xb, pw, pwt)
        ctx.conf = (wc.shape[0], wl.shape[0], wc.dtype, bc.dtype, x.dtype)
        return y

    @staticmethod
    def backward(ctx, gy):
        xb, w, wt = ctx.saved_tensors
        nc, nl, wdt, bdt, xdt = ctx.conf
        gyb = gy.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        gx = None
        if ctx.needs_input_grad[0]:
            gx = nat.conv2d_same(gyb, wt, None, dilation=1, relu=False, variant=7).to(xdt)
        partial = nat.channel_sums_partial(gyb)              # per-workgroup channel sums; the weight gradient's reduction launch adds them
        got = nat.conv3x3_wgrad(xb, gyb, bias_partial=partial)
        if got is None:
            raise RuntimeError("packed predictor head: weight-gradient geometry not covered")
        gw, gb = got if partial is not None else (got, gyb.float().sum(dim=(0, 2, 3)))
        return (gx, gw[:nc].to(wdt), gb[:nc].to(bdt), gw[nc:nc + nl].to(wdt), gb[nc:nc + nl].to(bdt), None, None, None)


class _AssembleTrainFn(torch.autograd.Function):
    """Reshape + Concatenate + softmax + AnchorBoxes + Concatenate of the TRAINING step (models/keras_ssd300.py:363-419) as one autograd
    node over the packed head maps: forward = ssdhip_assemble_predictions_strided_bf16 (the inference path's one-launch assembly),
    backward = ssdhip_assemble_predictions_backward_bf16 (softmax backward and the scatter into the packed layout, one launch) --
    instead of six slices, three concatenations, a softmax and an index_select forward and their ~15 kernels backward."""

    @staticmethod
    def forward(ctx, anchors, n_classes, n_boxes, *ys):
        pred = nat.assemble_predictions([y.detach() for y in ys], [None] * len(ys), [None] * len(ys), [None] * len(ys), list(n_boxes),
                                        anchors, n_classes)
        ctx.save_for_backward(pred)
        ctx.conf = (n_classes, tuple(n_boxes), tuple(tuple(y.shape) for y in ys))
        return pred

    @staticmethod
    def backward(ctx, g):
        (pred,) = ctx.saved_tensors
        n_classes, n_boxes, shapes = ctx.conf
        grads = nat.assemble_predictions_backward(g.float(), pred, shapes, n_boxes, n_classes)
        return (None, None, None) + tuple(grads)


class _MaxPoolFn(torch.autograd.Function):
    """max_pool2d of a bf16 NHWC map in the training step: libssdhip forward (one pass) and backward (gather, deterministic)."""

    @staticmethod
    def forward(ctx, x, kernel, stride, pad, ceil_mode):
        y = nat.bias_act_maxpool(x, None, kernel, stride, pad, ceil_mode, relu=False)
        ctx.save_for_backward(x)
        ctx.conf = (kernel, stride, pad)
        return y

    @staticmethod
    def backward(ctx, gy):
        (x,) = ctx.saved_tensors
        kernel, stride, pad = ctx.conf
        return nat.maxpool_bwd(x, gy.to(torch.bfloat16), kernel, stride, pad), None, None, None, None


def _nhwc(t):
    """t as a bf16 tensor whose memory is NHWC (a no-op for what the framework's channels_last convolutions return)."""
    t = t.to(torch.bfloat16)
    if not t.permute(0, 2, 3, 1).is_contiguous():
        t = t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    return t


class _BnEluPoolFn(torch.autograd.Function):
    """BatchNormalization (batch statistics, moving-average update) -> ELU [-> MaxPooling2D(2, 2) 'valid'] behind a convolution of SSD7's
    training step as one autograd node (csrc/ssdhip_bntrain.hip): three libssdhip launches forward, three backward, instead of the
    framework's batch_norm, elu and max_pool2d and their backward kernels.  Saves the convolution's output y, mean, invstd, gamma and
    beta -- no ELU output or mask: v is recomputed from y.  Returns (full | None, pooled | None, running_mean, running_var); the
    buffers are updated in place (marked dirty, so they are outputs) and take no gradient."""

    @staticmethod
    def forward(ctx, y, gamma, beta, running_mean, running_var, momentum, eps, pool, keep_full):
        y = _nhwc(y.detach())
        full, pooled, mean, invstd = nat.bn_elu_train_forward(y, gamma.detach(), beta.detach(), running_mean, running_var, momentum, eps,
                                                              pool, keep_full)
        ctx.mark_dirty(running_mean, running_var)
        ctx.mark_non_differentiable(running_mean, running_var)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(y, mean, invstd, gamma, beta)
        return full, pooled, running_mean, running_var

    @staticmethod
    def backward(ctx, g_full, g_pooled, _g_mean, _g_var):
        y, mean, invstd, gamma, beta = ctx.saved_tensors
        if g_full is None and g_pooled is None:
            return (None,) * 9
        dy, dgamma, dbeta = nat.bn_elu_train_backward(y, mean, invstd, gamma.detach(), beta.detach(),
                                                      None if g_full is None else _nhwc(g_full),
                                                      None if g_pooled is None else _nhwc(g_pooled))
        return dy, dgamma.to(gamma.dtype), dbeta.to(beta.dtype), None, None, None, None, None, None


class _Ssd7ConvFn(torch.autograd.Function):
    """A trunk convolution of SSD7's training step as one autograd node over libssdhip: forward = the block's MFMA kernel with the plain
    epilogue (convolution + bias, csrc/ssdhip_convbn.hip); backward = the same kernel on dL/dy with the transposed, tap-flipped filter
    image where the input needs a gradient (the 5 x 5 first layer's never does), and the weight / bias gradient of
    csrc/ssdhip_wgrad7.hip, written in the parameters' own dtype and memory order -- no framework op on either side.
    `image` / `flipped`: the layer's packed filters, refreshed by the model once per step (`nat.ssd7_pack_filters`); they are the
    model's buffers, not saved tensors.  Saves x -- the previous block's output, alive anyway -- and nothing derived; of the weight it
    keeps the parameter itself (no copy), for the gradient's layout and for this check: `flipped` is rewritten by every forward, so the
    data gradient is only right while the weights are the ones this forward saw.  Gradient accumulation over unchanged weights is
    fine; a backward that runs after an in-place weight update raises instead of using the newer filters."""

    @staticmethod
    def forward(ctx, x, weight, bias, image, flipped):
        x = _nhwc(x.detach())
        ctx.save_for_backward(x)
        ctx.flipped, ctx.weight, ctx.version = flipped, weight, weight._version
        return nat.ssd7_conv_bias(x, image, bias.detach(), weight.shape[0], weight.shape[2])

    @staticmethod
    def backward(ctx, gy):
        (x,) = ctx.saved_tensors
        weight = ctx.weight
        gy = _nhwc(gy)
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            if ctx.flipped is None:
                raise RuntimeError("_Ssd7ConvFn: the first layer has no data gradient (its input must not require one)")
            if weight._version != ctx.version:
                raise RuntimeError("_Ssd7ConvFn: the weights changed in place between this forward and its backward; the data "
                                   "gradient's filter image follows the newest forward")
            gx = nat.ssd7_conv_bias(gy, ctx.flipped, None, x.shape[1], weight.shape[2])
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            gw, gb = nat.ssd7_conv_wgrad(x, gy, weight.shape[2], like=weight)
        return gx, (gw if ctx.needs_input_grad[1] else None), (gb if ctx.needs_input_grad[2] else None), None, None


class _Ssd7HeadFn(torch.autograd.Function):
    """The two predictor heads of one source map of SSD7's training step as one autograd node over libssdhip (csrc/ssdhip_heads7.hip):
    the filters [conf | loc | zero rows] up to 48 output channels run as ONE convolution.  Forward = the blocks' MFMA kernel with the
    plain epilogue on the packed image and the packed bias; data gradient = the same kernel on dL/dy with the flipped image; parameter
    gradients = `nat.ssd7_head_wgrad`, which writes the four gradients in the parameters' own dtype and memory order and drops the
    padding rows -- no framework op on either side.  Returns the packed (B, 48, h, w) bf16 map with NHWC memory, which
    `_AssembleTrainFn` consumes.
    `image` / `flipped` / `packed_bias`: the model's buffers, rewritten from the current parameters once per step
    (`nat.ssd7_pack_heads`); they are not saved tensors.  As in `_Ssd7ConvFn`, a backward that runs after an in-place change of either
    filter raises instead of using the newer flipped image."""

    @staticmethod
    def forward(ctx, x, conf_w, conf_b, loc_w, loc_b, image, flipped, packed_bias):
        x = _nhwc(x.detach())
        ctx.save_for_backward(x)
        ctx.flipped, ctx.filters, ctx.versions = flipped, (conf_w, loc_w), (conf_w._version, loc_w._version)
        return nat.ssd7_conv_bias(x, image, packed_bias, nat.SSD7_HEAD_CP, 3)

    @staticmethod
    def backward(ctx, gy):
        (x,) = ctx.saved_tensors
        conf_w, loc_w = ctx.filters
        gy = _nhwc(gy)
        gx = None
        if ctx.needs_input_grad[0]:
            if (conf_w._version, loc_w._version) != ctx.versions:
                raise RuntimeError("_Ssd7HeadFn: the weights changed in place between this forward and its backward; the data "
                                   "gradient's filter image follows the newest forward")
            gx = nat.ssd7_conv_bias(gy, ctx.flipped, None, x.shape[1], 3)
        grads = (None,) * 4
        if any(ctx.needs_input_grad[1:5]):
            grads = tuple(g if need else None for g, need in zip(nat.ssd7_head_wgrad(x, gy, conf_w, loc_w), ctx.needs_input_grad[1:5]))
        return (gx,) + grads + (None, None, None)
