"""Which kernel every convolution layer is dispatched to, traced on the CPU (tests/test_conv_dispatch_cpu.py).

The per-layer selection of ssd_keras_amd.models only needs shapes: the layers here are bf16 modules and maps on the "meta" device (of
a tensor subclass that answers `is_cuda` with True, so the branches that ask are reached), `SSDModel._fused` / `_fused_train` are
patched to put a call on the inference or the training path, `SSDModel._pick` is patched to record its key and the candidates IN THE
ORDER OFFERED (the real one times them in that order and keeps the first of equal times) and to run every candidate once, and every
launching function of `ssd_keras_amd._native` is patched to record its name and arguments (a tensor as its dtype: the shapes follow from the case) and to return an empty tensor of the
result's shape.  `aten.convolution_backward`, the framework fallback of the gradients, is recorded through the subclass.  Nothing else is
patched, so the same file traces any revision of the package; tests/conv_dispatch_trace.json is what it recorded on the revision named
inside that file.
"""
import contextlib
import inspect
import json
import os
import types

import torch
from torch import nn

from ssd_keras_amd import _native as nat
from ssd_keras_amd.models._common import SSDModel, _ConvBiasActFn, _ConvBiasActPoolFn, _conv_input_weight_grads

TRACE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "conv_dispatch_trace.json")
RECORD_ENV = "CONV_DISPATCH_RECORD"          # set to the hash of the commit under trace: the test then WRITES the trace file

BATCHES = (1, 8, 16, 32)                     # 16: the threshold of the untimed rules; 1 / 32: both sides of few_tiles and of the image forms' 128 tiles

ENVS = (None, "SSDHIP_CONV=igemm", "SSDHIP_CONV=miopen", "SSDHIP_CONV=auto_miopen", "SSDHIP_PREFER=halo", "SSDHIP_NO_HALO=1",
        "SSDHIP_NO_IMAGE=1", "SSDHIP_IMAGE2=0", "SSDHIP_NO_SPLITK=1", "SSDHIP_GEMM_1X1=1", "SSDHIP_NO_OWN_DGRAD=1",
        "SSDHIP_NO_TAPS_BWD=1", "SSDHIP_NO_OWN_WGRAD=1", "SSDHIP_NO_MASKED_DGRAD=1", "SSDHIP_NO_C64_DGRAD=1", "SSDHIP_NO_POOL_KEEP=1",
        "SSDHIP_NO_CONV1_1_BWD=1", "SSDHIP_NO_MASKED_SUMS=1", "SSDHIP_NO_HALO_POOL_KEEP=1", "SSDHIP_NO_FUSED_POOL_BWD=1")


def _geometries():
    """name -> (Cin, Cout, k, stride, padding, dilation, groups, map side): every distinct convolution geometry of SSD300 and SSD512
    (models/keras_ssd300.py, keras_ssd512.py), the 3 -> 64 first layer, a predictor head (84 = 4 boxes x 21 classes), SSD512's 4 x 4
    conv10_2 and a grouped layer -- the last two fall to the framework."""
    g = {}
    for tag, sides in (("300", (300, 150, 75, 38, 19)), ("512", (512, 256, 128, 64, 32))):
        s1, s2, s3, s4, s5 = sides
        g.update({
            "conv1_1@" + tag: (3, 64, 3, 1, 1, 1, 1, s1), "conv1_2@" + tag: (64, 64, 3, 1, 1, 1, 1, s1),
            "conv2_1@" + tag: (64, 128, 3, 1, 1, 1, 1, s2), "conv2_2@" + tag: (128, 128, 3, 1, 1, 1, 1, s2),
            "conv3_1@" + tag: (128, 256, 3, 1, 1, 1, 1, s3), "conv3_2@" + tag: (256, 256, 3, 1, 1, 1, 1, s3),
            "conv4_1@" + tag: (256, 512, 3, 1, 1, 1, 1, s4), "conv4_2@" + tag: (512, 512, 3, 1, 1, 1, 1, s4),
            "conv5_1@" + tag: (512, 512, 3, 1, 1, 1, 1, s5), "fc6@" + tag: (512, 1024, 3, 1, 6, 6, 1, s5),
            "fc7@" + tag: (1024, 1024, 1, 1, 0, 1, 1, s5), "conv6_1@" + tag: (1024, 256, 1, 1, 0, 1, 1, s5),
            "conv6_2@" + tag: (256, 512, 3, 2, 1, 1, 1, s5), "head@" + tag: (512, 84, 3, 1, 1, 1, 1, s4)})
    g.update({
        "conv7_1@300": (512, 128, 1, 1, 0, 1, 1, 10), "conv7_2@300": (128, 256, 3, 2, 1, 1, 1, 10),
        "conv8_1@300": (256, 128, 1, 1, 0, 1, 1, 5), "conv8_2@300": (128, 256, 3, 1, 0, 1, 1, 5),
        "conv9_1@300": (256, 128, 1, 1, 0, 1, 1, 3), "conv9_2@300": (128, 256, 3, 1, 0, 1, 1, 3),
        "conv7_1@512": (512, 128, 1, 1, 0, 1, 1, 16), "conv7_2@512": (128, 256, 3, 2, 1, 1, 1, 16),
        "conv8_1@512": (256, 128, 1, 1, 0, 1, 1, 8), "conv8_2@512": (128, 256, 3, 2, 1, 1, 1, 8),
        "conv9_1@512": (256, 128, 1, 1, 0, 1, 1, 4), "conv9_2@512": (128, 256, 3, 2, 1, 1, 1, 4),
        "conv10_1@512": (256, 128, 1, 1, 0, 1, 1, 2), "conv10_2@512": (128, 256, 4, 1, 1, 1, 1, 2),
        "grouped@19": (128, 128, 3, 1, 1, 1, 2, 19)})
    return g


GEOMETRIES = _geometries()

# (link_in, wt, bias_partial, need_x, weight-gradient kernels decline) of the _conv_input_weight_grads entries
GRAD_FORMS = {"grads": (0, 0, 0, 1, 0), "grads+link": (1, 0, 0, 1, 0), "grads+wt": (0, 1, 0, 1, 0), "grads+partial": (0, 0, 1, 1, 0),
              "grads+link+wt+partial": (1, 1, 1, 1, 0), "grads-x": (0, 0, 1, 0, 0), "grads+declined": (0, 0, 1, 1, 1)}
# (relu, link_out: None absent / "out" present and unmasked / "masked" / "masked+partial", bias gradient wanted, need_x) of the
# _ConvBiasActFn.backward entries.  (A layer without ReLU holds no link_out: its forward drops it.)
LINK_OUT = (None, "out", "masked", "masked+partial")
BWD_FORMS = {"bwd%s%s%s%s" % ("" if relu else "_lin", "+" + link if link else "", "" if gb else "-gb", "" if need_x else "-x"):
             (relu, link, gb, need_x)
             for relu in (1, 0) for link in (LINK_OUT if relu else (None,)) for gb in (1, 0) for need_x in (1, 0)}
# (link_in, bias gradient wanted) of the _ConvBiasActPoolFn.backward entries
POOL_BWD_FORMS = {"pool_bwd": (0, 1), "pool_bwd+link": (1, 1), "pool_bwd-gb": (0, 0)}
ENTRIES = (("act_relu", "act_lin", "pool_ceil", "pool_floor", "pool_3_1_1", "thunk", "train_pool") + tuple(GRAD_FORMS) + tuple(BWD_FORMS)
           + tuple(POOL_BWD_FORMS))


class _Map(torch.Tensor):
    """A tensor without storage that says it lives on the GPU."""
    is_cuda = property(lambda self: True)
    on_convolution_backward = None               # the framework fallback of the gradients reports here (it still runs: shapes only)

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        if func is torch.ops.aten.convolution_backward and cls.on_convolution_backward is not None:
            cls.on_convolution_backward(*args)
        return super().__torch_function__(func, types, args, kwargs or {})


def _map(shape, dtype=torch.bfloat16, channels_last=True):
    t = torch.empty(tuple(int(n) for n in shape), dtype=dtype, device="meta")
    if channels_last and t.dim() == 4:
        t = t.contiguous(memory_format=torch.channels_last)
    return torch.Tensor._make_subclass(_Map, t)


_BATCH = [None]                              # the batch size of the running case: written "B" in shapes, so that batches share outcomes


def _desc(v):
    """What the trace keeps of a value: a tensor's dtype (shapes follow from the case), a 4-int shape with the batch as "B"."""
    if isinstance(v, torch.Tensor):
        return str(v.dtype).replace("torch.", "").replace("bfloat", "bf").replace("float", "f")
    if isinstance(v, (list, tuple)):
        if len(v) == 4 and all(type(u) is int for u in v):
            return ["B" if v[0] == _BATCH[0] else v[0]] + list(v[1:])
        return [_desc(u) for u in v]
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    return type(v).__name__


class _Unexpected(Exception):
    pass


class _Env(dict):
    """os.environ for one case: remembers which names were looked up (a switch that a case never reads cannot change its outcome)."""

    def __init__(self, base):
        super().__init__(base)
        self.read = set()

    def get(self, name, default=None):
        self.read.add(name)
        return super().get(name, default)

    def __getitem__(self, name):
        self.read.add(name)
        return super().__getitem__(name)

    def __contains__(self, name):
        self.read.add(name)
        return super().__contains__(name)


def _out(n, k, s, p, d):
    return (n + 2 * p - d * (k - 1) - 1) // s + 1


def _conv_result(a, pool=False):
    b, _, h, w = a["x"].shape
    cout, _, k, _ = a["weight"].shape
    s, p, d = a.get("stride", 1), a.get("padding", (a.get("dilation", 1) or 1) * (k // 2)), a.get("dilation", 1)
    ho, wo = _out(h, k, s, p, d), _out(w, k, s, p, d)
    if pool:
        ho, wo = (ho + 1) // 2, (wo + 1) // 2
    return _map((b, cout, ho, wo))


def _pool_out(n, k, s, p, ceil_mode):
    if ceil_mode:
        o = -(-(n + 2 * p - k) // s) + 1
        return o - 1 if (o - 1) * s >= n + p else o
    return (n + 2 * p - k) // s + 1


def _wgrad_result(a, k, state):
    if state["decline"]:
        return None
    gw = _map((a["dy"].shape[1], a["x"].shape[1], k, k), torch.float32)
    return gw if a["bias_partial"] is None else (gw, _map((a["dy"].shape[1],), torch.float32))


def _slab(a):
    return a["weight"].shape[0] % 128 == 0 and a["weight"].shape[1] % 128 == 0


def _halo_masked(a, st):
    if not _slab(a):
        return None
    y = _conv_result(a)
    return (y, _map((8, a["weight"].shape[0]), torch.float32)) if a["sums"] else y


def _sums(c, reduce):
    """The channel sums of a C-channel map ([rows, C] partials, or [C]); None where csrc/ssdhip_train.hip's passes decline the count."""
    if c % 8 or 256 % (c // 8):
        return None
    return _map((c,) if reduce else (8, c), torch.float32, False)


def _masked_and_sums(full, reduce):
    sums = _sums(full.shape[1], reduce)
    return None if sums is None else (_map(full.shape), sums)


# what a launching function returns here: empty tensors of the real result's shape (a: its arguments by name, defaults filled in)
RESULTS = {
    "conv2d_same": lambda a, st: _conv_result(a),
    "conv2d": lambda a, st: _conv_result(a),
    "conv3x3_image": lambda a, st: _conv_result(a),
    "conv2d_image": lambda a, st: _conv_result(a),
    "conv3x3_cin3": lambda a, st: _conv_result(a),
    "conv3x3_c64": lambda a, st: _conv_result(a, a["pool"]),
    "conv3x3_halo": lambda a, st: _conv_result(a, a["pool"]),
    "conv2d_same_pool2": lambda a, st: _conv_result(a, True),
    "conv3x3_c64_pool_keep": lambda a, st: (_conv_result(a), _conv_result(a, True)),
    "conv3x3_halo_pool_keep": lambda a, st: (_conv_result(a), _conv_result(a, True)) if _slab(a) else None,
    "conv1_block": lambda a, st: _conv_result(a, a["pool"]),
    "bias_act": lambda a, st: _map(a["x"].shape),
    "bias_act_maxpool": lambda a, st: _map((a["x"].shape[0], a["x"].shape[1],
                                            _pool_out(a["x"].shape[2], a["kernel"], a["stride"], a["pad"], a["ceil_mode"]),
                                            _pool_out(a["x"].shape[3], a["kernel"], a["stride"], a["pad"], a["ceil_mode"]))),
    "embed_strided": lambda a, st: _map((a["gy"].shape[0], a["gy"].shape[1], a["h"], a["w"])),
    "conv3x3_halo_masked": _halo_masked,
    "conv3x3_wgrad": lambda a, st: _wgrad_result(a, 3, st),
    "conv1x1_wgrad": lambda a, st: _wgrad_result(a, 1, st),
    "conv3x3_taps_wgrad": lambda a, st: _wgrad_result(a, 3, st),
    "relu_bwd_bias": lambda a, st: _masked_and_sums(a["gy"], a["reduce"]),
    "maxpool2_relu_bwd_bias": lambda a, st: _masked_and_sums(a["y"], a["reduce"]),
    "channel_sums_partial": lambda a, st: _sums(a["gy"].shape[1], False),
    "row_sums": lambda a, st: _map(a["partial"].shape[1:], torch.float32),
    "conv1_1_backward": lambda a, st: (_map((64, 3, 3, 3), torch.float32), _map((64,), torch.float32)),
}
HOST_ONLY = ("conv2d_image_supported", "conv3x3_image_supported", "conv3x3_halo_plan", "assemble_backward_supported", "load",
             "lib_path", "check", "require_cuda")


class Tracer:
    """One SSDModel base instance with the seams patched; `run(entry, geometry, batch)` returns the JSON-able outcome."""

    def __init__(self):
        self.model = SSDModel((300, 300, 3), 20, "training", 0.0, None, None, None, 0.01, 0.45, 200, 400, "centroids", True)
        self.events = []
        self.state = {"path": None, "decline": False}
        self.convs = {}

    # -- the patches ---------------------------------------------------------------------------------------------------------------
    def _stub(self, name, real):
        sig = inspect.signature(real)
        params = list(sig.parameters)

        def stub(*args, **kwargs):
            if name not in RESULTS:
                raise _Unexpected(name)
            bound = sig.bind(*args, **kwargs)
            bound.apply_defaults()
            a = dict(bound.arguments)
            self.events.append([name, {p: _desc(a[p]) for p in params}])
            first = params[0]
            if first != "x" and "x" not in a:
                a["x"] = a[first]
            return RESULTS[name](a, self.state)
        return stub

    def _pick(self, model, key, candidates):
        ev = {"pick": _desc(key), "names": list(candidates), "calls": {}}
        outer = self.events
        for name, fn in candidates.items():
            self.events = []
            try:
                fn()
            except _Unexpected as e:
                self.events.append(["unexpected", str(e)])
            ev["calls"][name] = self.events
        self.events = outer
        self.events.append(ev)
        hit = SSDModel._conv_choice.get(key)             # the cache as the real _pick reads it; nothing timed: the LAST candidate otherwise
        return hit if hit is not None else ev["names"][-1]

    def _conv_bwd(self, gy, x, w, bias_sizes, stride, padding, dilation, transposed, output_padding, groups, masks):
        self.events.append(["aten.convolution_backward", {"grad_output": _desc(gy), "input": _desc(x), "weight": _desc(w),
                                                          "stride": list(stride), "padding": list(padding), "dilation": list(dilation),
                                                          "groups": groups, "output_mask": list(masks)}])

    @contextlib.contextmanager
    def patched(self):
        saved_nat = {}
        for name, real in list(vars(nat).items()):
            if (inspect.isfunction(real) and real.__module__ == nat.__name__ and not name.startswith("_") and name not in HOST_ONLY):
                saved_nat[name] = real
                setattr(nat, name, self._stub(name, real))
        saved_cls = {n: SSDModel.__dict__[n] for n in ("_pick", "_fused", "_fused_train", "_conv_choice")}
        tracer = self
        SSDModel._pick = lambda model, key, candidates: tracer._pick(model, key, candidates)
        SSDModel._fused = lambda model, x, conv=None: tracer.state["path"] == "inference"
        SSDModel._fused_train = lambda model, x, conv: tracer.state["path"] == "training"
        _Map.on_convolution_backward = self._conv_bwd
        self.real_environ = os.environ                   # every case runs under a copy without SSDHIP_* variables (see run)
        try:
            yield self
        finally:
            os.environ = self.real_environ
            _Map.on_convolution_backward = None
            for n, v in saved_cls.items():
                setattr(SSDModel, n, v)
            for name, real in saved_nat.items():
                setattr(nat, name, real)

    # -- the cases -----------------------------------------------------------------------------------------------------------------
    def conv(self, geometry):
        if geometry not in self.convs:
            cin, cout, k, s, p, d, groups, _side = GEOMETRIES[geometry]
            self.convs[geometry] = nn.Conv2d(cin, cout, k, stride=s, padding=p, dilation=d, groups=groups, device="meta",
                                             dtype=torch.bfloat16)
        return self.convs[geometry]

    def run(self, entry, geometry, batch, env=None):
        """The outcome of one case under `env` ("NAME=value" or None) alone: {"events": [...], "result": ..., "keys": the autotune keys
        that the events call K0, K1, ...}; `self.read` then holds the names of the environment variables the case looked up."""
        os.environ = _Env({k: v for k, v in self.real_environ.items() if not k.startswith("SSDHIP_")})
        if env:
            dict.__setitem__(os.environ, *env.split("="))
        self.read = os.environ.read
        SSDModel._conv_choice = {}
        self.events = []
        _BATCH[0] = batch
        self.state.update(path="inference", decline=False)
        cin, cout, k, s, p, d, groups, side = GEOMETRIES[geometry]
        conv, x, m = self.conv(geometry), _map((batch, cin, side, side)), self.model
        try:
            if entry == "act_relu":
                res = _desc(m.conv_act(conv, x, relu=True))
            elif entry == "act_lin":
                res = _desc(m.conv_act(conv, x, relu=False))
            elif entry == "pool_ceil":
                res = _desc(m.conv_act_pool(conv, x, 2, 2, ceil_mode=True))
            elif entry == "pool_floor":
                res = _desc(m.conv_act_pool(conv, x, 2, 2, ceil_mode=False))
            elif entry == "pool_3_1_1":
                res = _desc(m.conv_act_pool(conv, x, 3, 1, pad=1))
            elif entry == "conv1_block":
                c1 = self.conv("conv1_1@" + geometry.split("@")[1])
                res = _desc(m.conv1_block_pool(c1, conv, _map((batch, 3, side, side))))
            elif entry == "thunk":
                res = self._thunk(conv, x)
            elif entry == "train_pool":
                self.state["path"] = "training"
                with torch.enable_grad():
                    res = _desc(m.conv_act_pool(conv, x, 2, 2, ceil_mode=True))
            elif entry in GRAD_FORMS:
                res = self._grads(entry, conv, x)
            else:
                res = self._backward(entry, conv, x)
        except _Unexpected as e:
            res = "unexpected call: %s" % e
        keys = []
        return json.loads(json.dumps({"events": _name_keys(self.events, keys), "result": res, "keys": keys}))

    def _thunk(self, conv, x):
        """The names offered, their order and the key; the name returned, also when the cache holds a winner of the inference path that
        the training step does not offer."""
        self.state["path"] = "training"
        run, name = self.model._train_thunk(conv, x, True)
        res = {"name": name}
        picks = [e for e in self.events if isinstance(e, dict)]
        if run is not None:
            before = len(self.events)
            run(x, conv.weight, conv.bias)
            res["launch"] = self.events[before:]
            del self.events[before:]
        if picks:
            key = picks[0]["pick"]
            as_tuple = lambda v: tuple(as_tuple(u) for u in v) if isinstance(v, list) else (x.shape[0] if v == "B" else v)
            SSDModel._conv_choice = {as_tuple(key): "splitk"}
            before = len(self.events)
            res["name_when_cache_holds_splitk"] = self.model._train_thunk(conv, x, True)[1]
            del self.events[before:]
        return res

    def _grads(self, entry, conv, x):
        link, wt, partial, need_x, decline = GRAD_FORMS[entry]
        self.state.update(path="training", decline=bool(decline))
        cin, cout, k, s, p, d = conv.in_channels, conv.out_channels, conv.kernel_size[0], conv.stride[0], conv.padding[0], conv.dilation[0]
        gy = _map((x.shape[0], cout, _out(x.shape[2], k, s, p, d), _out(x.shape[3], k, s, p, d)))
        link_in = None
        if link:
            with torch.enable_grad():
                link_in = self.model.relu_link()
        got = _conv_input_weight_grads(gy, x, conv.weight, conv.stride, conv.padding, conv.dilation, bool(need_x),
                                       _map((cin, cout, k, k)) if wt else None,
                                       _map((8, cout), torch.float32, False) if partial else None, link_in)
        return {"grads": _desc(got), "link_masked": bool(link_in.masked) if link_in is not None else None,
                "link_partial": _desc(link_in.partial) if link_in is not None else None}

    def _backward(self, entry, conv, x):
        """`backward` of the layer's autograd node [of the layer + pool node], called as the plain static method it is on what its
        forward would have saved: the launches, the three leading gradients, how many results and the link's state afterwards."""
        self.state["path"] = "training"
        cin, cout, k, s, p, d = conv.in_channels, conv.out_channels, conv.kernel_size[0], conv.stride[0], conv.padding[0], conv.dilation[0]
        y = _map((x.shape[0], cout, _out(x.shape[2], k, s, p, d), _out(x.shape[3], k, s, p, d)))
        with torch.enable_grad():
            link = self.model.relu_link()
        # (dtypes that every gradient has to be cast to: the kernels return bf16 dL/dx and float32 dL/dw, dL/db)
        dtypes = (torch.bfloat16, torch.bfloat16, torch.float32)
        if entry in BWD_FORMS:
            relu, state, gb, need_x = BWD_FORMS[entry]
            if state is None:
                link = None
            else:
                link.masked = state.startswith("masked")
                link.partial = _map((8, cout), torch.float32, False) if state.endswith("partial") else None
            ctx = types.SimpleNamespace(saved_tensors=(x, conv.weight, y if relu else None, None), links=(None, link),
                                        conf=(conv.stride, conv.padding, conv.dilation, bool(relu)) + dtypes,
                                        needs_input_grad=(bool(need_x), True, bool(gb)) + (False,) * 10)
            node, g_out = _ConvBiasActFn, y
        else:
            link_in, gb = POOL_BWD_FORMS[entry]
            link = link if link_in else None
            ctx = types.SimpleNamespace(saved_tensors=(x, conv.weight, y, None), link_in=link, conf=(conv.stride, conv.padding, conv.dilation) + dtypes,
                                        needs_input_grad=(True, True, bool(gb)) + (False,) * 8)
            node, g_out = _ConvBiasActPoolFn, _map((y.shape[0], cout, (y.shape[2] + 1) // 2, (y.shape[3] + 1) // 2))
        try:
            got = node.backward(ctx, g_out)
            res = {"grads": _desc(got[:3]), "results": len(got)}
        except RuntimeError as e:                        # (the pooled node on a channel count its one-pass backward declines)
            res = {"raises": "RuntimeError: %s" % e}
        return dict(res, link_masked=bool(link.masked) if link is not None else None,
                    link_partial=_desc(link.partial) if link is not None else None)


def _name_keys(events, keys):
    """The events with every autotune key replaced by its place in `keys`: what is left no longer depends on the layer's size."""
    out = []
    for ev in events:
        if isinstance(ev, dict):
            if ev["pick"] not in keys:
                keys.append(ev["pick"])
            ev = dict(ev, pick="K%d" % keys.index(ev["pick"]), calls={n: _name_keys(c, keys) for n, c in ev["calls"].items()})
        out.append(ev)
    return out


def applies(entry, geometry):
    if entry == "pool_floor":
        return GEOMETRIES[geometry][7] % 2 == 1          # ceil_mode=False on an odd map: no fused pooling epilogue
    if entry == "conv1_block":
        return geometry.startswith("conv1_2@")
    if entry in GRAD_FORMS or entry in BWD_FORMS or entry in POOL_BWD_FORMS:
        return GEOMETRIES[geometry][6] == 1              # (a grouped layer never reaches the gradients: SSDModel._fused_train)
    return True


def case_ids():
    return ["%s|%s" % (entry, geometry) for geometry in GEOMETRIES for entry in ENTRIES + ("conv1_block",) if applies(entry, geometry)]


def run_case(tracer, cid, batch, envs=ENVS):
    """{env: outcome} of one case at one batch size, for the default environment (None) and every env of `envs` whose variable the
    case reads there -- the others cannot change the outcome and are left out."""
    entry, geometry = cid.split("|")
    got = {None: tracer.run(entry, geometry, batch)}
    read = set(tracer.read)
    for env in envs:
        if env and env.split("=")[0] in read:
            got[env] = tracer.run(entry, geometry, batch, env)
    return got


def _intern(v, table, index):
    s = json.dumps(v, sort_keys=True)
    if s not in index:
        index[s] = len(table)
        table.append(v)
    return index[s]


def _launches(events, fn):
    """The events with fn applied to every launch (a [name, arguments] pair), inside the candidates of a pick too."""
    return [dict(ev, calls={n: _launches(c, fn) for n, c in ev["calls"].items()}) if isinstance(ev, dict) else fn(ev) for ev in events]


def _with_launches(o, fn):
    o = dict(o, events=_launches(o["events"], fn))
    if isinstance(o["result"], dict) and "launch" in o["result"]:
        o["result"] = dict(o["result"], launch=_launches(o["result"]["launch"], fn))
    return o


def trace():
    """{"launches": the distinct launches, "outcomes": the distinct outcomes without their keys, a launch being its place in "launches",
    "keys": the distinct key lists, "results": the distinct [outcome, keys] pairs, "cases": {case id: [results under the default
    environment, {place of an environment in ENVS: results where any differs}]}}; results: one per batch size, or one number for all."""
    tables = {"launches": [], "outcomes": [], "keys": [], "results": []}
    index = {n: {} for n in tables}
    cases = {}
    with Tracer().patched() as t, torch.no_grad():
        for cid in case_ids():
            rows = {}
            for b in BATCHES:
                got = run_case(t, cid, b)
                for env in ENVS:
                    o = _with_launches(got.get(env, got[None]), lambda ev: _intern(ev, tables["launches"], index["launches"]))
                    k = _intern(o.pop("keys"), tables["keys"], index["keys"])
                    pair = [_intern(o, tables["outcomes"], index["outcomes"]), k]
                    rows.setdefault(env, []).append(_intern(pair, tables["results"], index["results"]))
            rows = {env: r[0] if len(set(r)) == 1 else r for env, r in rows.items()}
            cases[cid] = [rows[None], {str(ENVS.index(env)): r for env, r in rows.items() if env and r != rows[None]}]
    return dict(tables, cases=cases)


def recorded_outcome(rec, cid, batch, env):
    """The outcome the trace file holds for a case, in the form `Tracer.run` returns."""
    base, differing = rec["cases"][cid]
    row = differing.get(str(ENVS.index(env)), base)
    o, k = rec["results"][row[BATCHES.index(batch)] if isinstance(row, list) else row]
    return dict(_with_launches(rec["outcomes"][o], lambda i: rec["launches"][i]), keys=rec["keys"][k])


def _rows(items, width=150):
    """JSON items, comma-separated, as many to a line as fit `width`."""
    lines = [""]
    for item in items:
        if lines[-1] and len(lines[-1]) + len(item) > width:
            lines.append("")
        lines[-1] += item + ","
    return "\n".join(lines).rstrip(",")


def write_trace(commit):
    rec = trace()
    dumps = lambda v: json.dumps(v, separators=(",", ":"))
    with open(TRACE, "w") as f:
        f.write('{"recorded_on_commit": %s, "batches": %s,\n"environments": %s,\n' % (
            json.dumps(commit), json.dumps(list(BATCHES)), json.dumps([e or "default" for e in ENVS])))
        for name in ("launches", "outcomes", "keys", "results"):
            f.write('"%s": [\n%s\n],\n' % (name, _rows(dumps(v) for v in rec[name])))
        f.write('"cases": {\n%s\n}}\n' % _rows("%s:%s" % (json.dumps(k), dumps(v)) for k, v in rec["cases"].items()))
