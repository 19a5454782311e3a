"""The bf16 shadow set of a model with float32 master weights: what the MFMA kernels of the training step read."""
import torch
from torch import nn

from .. import _native as nat
from ..optimizers import _bump_versions
from ._conv_select import geometry_of, own_dgrad


class ShadowSet:
    """bf16 copies of every convolution's float32 master weights in the layouts the MFMA kernels read (csrc/ssdhip_optim.hip):
    channels_last filters (`cl`), their transposed / tap-flipped twin where the layer's data gradient runs on our kernels (`tr`, written
    at (row count, row offset) `tr_arg`), the bias; the conf and loc heads of a source map as ROWS OF ONE packed tensor (`packs[l]` =
    [conf | loc | zero rows up to a multiple of 128] filters, bias, transposed filters, n_conf, n_loc: what _PackedHeadFn multiplies),
    so that nothing is concatenated, flipped or re-laid-out per step.  `index` maps id(conv) to its slot."""

    def __init__(self, model, device):
        self.device = device
        self.key = self.table = self.table_key = None    # versions of the masters at the last refresh; the launch's pointer table
        convs = [m for m in model.modules() if isinstance(m, nn.Conv2d) and m.bias is not None]
        index = {id(c): i for i, c in enumerate(convs)}
        cl, tr, bias, tr_arg = [None] * len(convs), [None] * len(convs), [None] * len(convs), [(0, 0)] * len(convs)
        packs = {}
        heads = list(zip(getattr(model, "conf_heads", []), getattr(model, "loc_heads", [])))
        with torch.no_grad():
            for l, (ch, lh) in enumerate(heads):
                same = lambda c: (isinstance(c, nn.Conv2d) and c.kernel_size == (3, 3) and c.stride == (1, 1) and c.padding == (1, 1)
                                  and c.dilation == (1, 1) and c.groups == 1 and c.bias is not None and id(c) in index)
                if not (same(ch) and same(lh) and ch.in_channels == lh.in_channels and ch.in_channels % 128 == 0):
                    continue
                nc, nl, cin = ch.out_channels, lh.out_channels, ch.in_channels
                cp = -(-(nc + nl) // 128) * 128
                pw = torch.zeros((cp, cin, 3, 3), dtype=torch.bfloat16, device=device).contiguous(memory_format=torch.channels_last)
                pwt = torch.zeros((cin, cp, 3, 3), dtype=torch.bfloat16, device=device).contiguous(memory_format=torch.channels_last)
                pb = torch.zeros((cp,), dtype=torch.bfloat16, device=device)
                packs[l] = (pw, pb, pwt, nc, nl)
                for conv, lo, n in ((ch, 0, nc), (lh, nc, nl)):
                    i = index[id(conv)]
                    cl[i], bias[i], tr[i], tr_arg[i] = pw[lo:lo + n], pb[lo:lo + n], pwt, (cp, lo)
            for i, c in enumerate(convs):
                if cl[i] is not None:
                    continue
                cl[i] = torch.empty(tuple(c.weight.shape), dtype=torch.bfloat16, device=device).contiguous(memory_format=torch.channels_last)
                if cl[i].dim() == 4 and not cl[i].permute(0, 2, 3, 1).is_contiguous():          # size-1 dims can leave odd strides behind
                    cl[i] = torch.empty(tuple(c.weight.permute(0, 2, 3, 1).shape), dtype=torch.bfloat16, device=device).permute(0, 3, 1, 2)
                bias[i] = torch.empty((c.out_channels,), dtype=torch.bfloat16, device=device)
                if own_dgrad(geometry_of(c)):
                    o, ci, kh, kw = c.weight.shape
                    tr[i] = torch.empty((ci, kh, kw, o), dtype=torch.bfloat16, device=device).permute(0, 3, 1, 2)   # (I, O, kh, kw) channels_last
                    tr_arg[i] = (o, 0)
        dests, seen = [], set()                                   # every tensor the refresh launch writes, once (views share a counter)
        for t in cl + tr + bias + [u for pk in packs.values() for u in pk[:3]]:
            if t is None:
                continue
            base = t._base if t._base is not None else t
            if id(base) not in seen:
                seen.add(id(base))
                dests.append(base)
        self.convs, self.index, self.cl, self.tr, self.bias, self.tr_arg, self.packs, self.dests = convs, index, cl, tr, bias, tr_arg, packs, tuple(dests)

    def refresh(self):
        """Every bf16 copy up to date: ONE launch over all parameters when any of them changed.  The key holds the Parameter OBJECT,
        its storage and its version: an optimizer step bumps the version, `param.data = t` changes the storage,
        `conv.weight = nn.Parameter(...)` the object."""
        src = [c.weight for c in self.convs] + [c.bias for c in self.convs]
        key = tuple((id(t), t.data_ptr(), t._version) for t in src)
        if key != self.key:
            tkey = tuple((id(t), t.data_ptr(), tuple(t.stride())) for t in src)
            if self.table is None or self.table_key != tkey:             # the table holds raw pointers: rebuilt when a storage moved
                w = [(c.weight.detach(), self.cl[i], self.tr[i], self.tr_arg[i][0], self.tr_arg[i][1]) for i, c in enumerate(self.convs)]
                v = [(c.bias.detach().contiguous(), self.bias[i]) for i, c in enumerate(self.convs)]
                if any(b.data_ptr() != c.bias.data_ptr() for (b, _), c in zip(v, self.convs)):
                    raise RuntimeError("a convolution bias is not a contiguous tensor")
                self.table = nat.shadow_table(w, v, self.device)
                self.table_key = tkey
            nat.shadow_refresh(self.table)
            # the kernel rewrote the shadows in place behind autograd's back: their version counters move as an in-place tensor
            # op's would, so a backward whose forward saved the OLD filters raises instead of multiplying the new ones
            _bump_versions(self.dests)
            # Inside a stream capture the refresh is only RECORDED (it runs at every replay): the shadows are not fresh for the next
            # eager call, which must refresh them itself (tests/test_train_graph_gpu.py: the first eager step after a capture
            # multiplied the previous step's filters, 1.3e-3 off on the loss).
            if not torch.cuda.is_current_stream_capturing():
                self.key = key


def fresh(model, device):
    """The model's shadow set on `device`, up to date.  Inside raw_predictions the check runs once per forward pass (`_shadow_fresh`);
    a direct call of features() / conv_act() checks every time."""
    st = model.__dict__.get("_shadow_state")
    if st is None or st.device != device:
        st = model.__dict__["_shadow_state"] = ShadowSet(model, device)
    if not (model.__dict__.get("_in_forward", False) and model.__dict__.get("_shadow_fresh", False)):
        st.refresh()
        model.__dict__["_shadow_fresh"] = True
    return st
