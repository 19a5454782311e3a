"""The optimizers of the reference's training notebooks as torch optimizers whose step is ONE libssdhip launch over every parameter
instead of the framework's dozen multi-tensor launches (0.34 ms of an 11 ms SSD300 step, profiles/r05h_train_step_timeline.json).

`SGD` -- `keras.optimizers.SGD(lr=0.001, momentum=0.9, decay=0.0, nesterov=False)` (ssd300_training.ipynb:169; csrc/ssdhip_optim.hip,
sgd_momentum_kernel).  Update rule: torch.optim.SGD's (`buf = momentum * buf + grad`, `p -= lr * buf`), which is Keras's
(`v = momentum * v - lr * g`, `p += v`) for a constant learning rate; `weight_decay` adds `weight_decay * p` to the gradient first (Keras
expresses the same thing as `kernel_regularizer=l2(5e-4)` on the loss, models/keras_ssd300.py:274: gradient `2 * 5e-4 * W`).

`Adam` -- `keras.optimizers.Adam(lr=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-08, decay=0.0)`, the optimizer of every other notebook
(ssd7_training.ipynb:153; csrc/ssdhip_adam.hip).  Update rule: Keras 2.x `Adam.get_updates`, NOT torch.optim.Adam's --
`lr_t = lr * sqrt(1 - b2^t) / (1 - b1^t)`, `p -= lr_t * m / (sqrt(v) + epsilon)`: epsilon is added to the UNcorrected sqrt(v), 30 x the
effective epsilon of torch's rule at t = 1.  The step count, the running products b^t and every scalar of the update live in a state
block on the device that a tick kernel advances, so `step()` captured into a HIP graph replays with the bias correction of ITS step,
and `set_lr` changes the learning rate between replays.

In both, float32 parameters on a GPU with gradients of their own memory layout take the fused launch; anything else (CPU tensors, other
dtypes, SGD with momentum 0) the plain tensor expressions of the same rule."""
from __future__ import annotations

import math

import torch

from . import _native as nat


def _bump_versions(tensors):
    """What an in-place tensor op does to `_version`, for parameters a libssdhip kernel has just updated behind autograd's back."""
    try:
        torch._C._autograd._unsafe_set_version_counter(tuple(tensors), tuple(t._version + 1 for t in tensors))
    except (AttributeError, TypeError):                      # an older framework: a multi-tensor no-op bumps them too
        torch._foreach_add_(list(tensors), 0)


class _OneLaunchOptimizer(torch.optim.Optimizer):
    """What the one-launch optimizers share: which parameters are eligible, and the cache of their pointer tables."""

    _buffers = ()                                            # names of the per-parameter state tensors the kernel touches

    # The device tables hold RAW pointers (parameter, gradient, state buffers): everything that can replace one of those tensors
    # drops them, and the per-step key below covers all their addresses as well (the key used to hold the gradients'
    # addresses only -- `load_state_dict` after a step replaced the momentum buffers, the kernel kept updating the freed ones).
    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._tables = {}

    def __setstate__(self, state):
        super().__setstate__(state)
        self._tables = {}                                     # never pickled pointers: rebuilt on the next step

    def __getstate__(self):
        state = dict(super().__getstate__()) if hasattr(super(), "__getstate__") else dict(self.__dict__)
        state.pop("_tables", None)
        return state

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        self._tables = {}

    @staticmethod
    def _dense(t):
        return t.is_contiguous() or (t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last))

    @staticmethod
    def _same_order(g, p):
        """The two tensors walk memory in the same order: equal strides on every dimension that has more than one entry (a 1 x 1 filter
        is the same memory contiguous or channels_last; only the stride METADATA of its size-1 dimensions differs)."""
        return tuple(g.shape) == tuple(p.shape) and all(a == b for a, b, n in zip(g.stride(), p.stride(), p.shape) if n != 1)

    def _split(self, group, fusable=True):
        """The parameters of a group that have a gradient: {device: those that take the fused launch}, [the others]."""
        fused, rest = {}, []
        for p in group["params"]:
            g = p.grad
            if g is None:
                continue
            ok = (fusable and p.is_cuda and p.dtype == torch.float32 and g.dtype == torch.float32 and not g.is_sparse
                  and self._dense(p) and self._same_order(g, p) and p.data_ptr() % 16 == 0 and g.data_ptr() % 16 == 0)
            if ok:
                fused.setdefault(p.device, []).append(p)
            else:
                rest.append(p)
        return fused, rest

    def _key(self, group):
        """Which parameters have a gradient, and where the tensors the kernel touches live."""
        state, names = self.state, self._buffers
        key = []
        for p in group["params"]:
            g = p.grad
            if g is None:
                key.append(0)
                continue
            st = state[p] if p in state else ()
            key.append((g.data_ptr(), p.data_ptr()) + tuple(st[n].data_ptr() if n in st else 0 for n in names))
        return tuple(key)

    def _planned(self, gi, group, tag):
        """(tables, rest) of `_plan(gi, group)`, rebuilt only when a tensor moved (the tables hold raw pointers) or `tag` changed.
        Everything per-parameter that can be decided once is decided in `_plan`: the step itself is host-bound (~280 launches in
        11 ms), every microsecond of Python in it shows."""
        key = self._key(group)
        tabs = self.__dict__.setdefault("_tables", {})
        hit = tabs.get(gi)
        if hit is None or hit[0] != key or hit[1] != tag:
            plan = self._plan(gi, group)                     # (creates the missing state buffers: the key is taken again with them)
            hit = (self._key(group), tag) + plan
            tabs[gi] = hit
        return hit[2], hit[3]


_flat = lambda t: t.detach().as_strided((t.numel(),), (1,))


class SGD(_OneLaunchOptimizer):
    _buffers = ("momentum_buffer",)

    def __init__(self, params, lr=0.01, momentum=0.0, weight_decay=0.0, decay=0.0, nesterov=False):
        if lr < 0.0 or momentum < 0.0 or weight_decay < 0.0:
            raise ValueError("lr, momentum and weight_decay must be non-negative")
        if decay != 0.0 or nesterov:
            raise ValueError("the reference trains with decay=0.0, nesterov=False (ssd300_training.ipynb:169); neither is implemented")
        super().__init__(params, dict(lr=lr, momentum=momentum, weight_decay=weight_decay))
        self._tables = {}

    def _plan(self, gi, group):
        fused, rest = self._split(group, fusable=group["momentum"] != 0.0)
        tables = []
        for dev, ps in fused.items():
            bufs = []
            for p in ps:
                st = self.state[p]
                if "momentum_buffer" not in st:               # zeros: the first update is then buf = grad, as torch's clone(grad)
                    st["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                bufs.append(st["momentum_buffer"])
            tables.append((nat.sgd_table([_flat(p) for p in ps], [_flat(p.grad) for p in ps], [_flat(b) for b in bufs], dev), tuple(ps)))
        return tables, rest

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for gi, group in enumerate(self.param_groups):
            lr, mom, wd = group["lr"], group["momentum"], group["weight_decay"]
            tables, rest = self._planned(gi, group, mom)
            for table, ps in tables:
                nat.sgd_momentum_step(table, lr, mom, wd)
                _bump_versions(ps)                                  # caches keyed on `_version` (the bf16 shadows) must see the update
            for p in rest:
                g = p.grad
                if wd != 0.0:
                    g = g.add(p, alpha=wd)
                if mom != 0.0:
                    st = self.state[p]
                    buf = st.get("momentum_buffer")
                    if buf is None:
                        buf = st["momentum_buffer"] = torch.clone(g).detach()
                    else:
                        buf.mul_(mom).add_(g)
                    g = buf
                p.add_(g, alpha=-lr)
        return loss


class Adam(_OneLaunchOptimizer):
    """keras.optimizers.Adam with Keras's parameter names and defaults (`epsilon=None` is K.epsilon() = 1e-7; the notebooks pass 1e-08);
    `weight_decay` per group as in `SGD` (Keras's l2 kernel regulariser).  `lr` may change at any time -- through `param_groups` (a
    `torch.optim.lr_scheduler` does that; the next eager `step()` sends it to the device) or through `set_lr`, which is what a caller
    uses between two replays of a captured step; the other hyperparameters are fixed once the first step has been taken.

    A step inside `torch.cuda.graph` records the tick and the update launches only.  Nothing may be allocated there, so the moment
    buffers and the state block must exist: take an eager step first, or call `init_state()` with the gradients in place.
    `iterations` reads the device's count back (a synchronisation: for logging and checkpoints).  A device's count advances with the
    update launches on that device and the host's with the tensor expressions: in an optimizer that mixes both, a step in which no
    parameter of a device has a gradient leaves that device's count one behind (the notebooks' models never do that).
    `_fused = False` on an instance is a TEST HOOK: every parameter then goes through the tensor expressions, which is what the tests
    compare the kernel with."""

    _buffers = ("m", "v", "vhat")
    _BLOCK = "adam_state:"                                    # self.state[_BLOCK + device]: the device's state block, a uint8 tensor
    _HOST = "adam_host"                                       # self.state[_HOST]: the same scalars for the tensor-expression path
    _fused = True

    def __init__(self, params, lr=0.001, beta_1=0.9, beta_2=0.999, epsilon=None, decay=0.0, amsgrad=False, weight_decay=0.0):
        if epsilon is None:
            epsilon = 1e-7
        defaults = dict(lr=lr, beta_1=beta_1, beta_2=beta_2, epsilon=epsilon, decay=decay, amsgrad=bool(amsgrad), weight_decay=weight_decay)
        self._check(defaults)
        super().__init__(params, defaults)
        self._tables, self._seen = {}, {}
        for group in self.param_groups:
            self._check(group)
        self._check_groups()

    def _check_groups(self):
        if len(self.param_groups) > nat.ADAM_MAX_GROUPS:
            raise ValueError("at most %d parameter groups (the device state block's size)" % nat.ADAM_MAX_GROUPS)

    @staticmethod
    def _check(group):
        if not (group["lr"] >= 0.0 and group["epsilon"] >= 0.0 and group["decay"] >= 0.0 and group["weight_decay"] >= 0.0):
            raise ValueError("lr, epsilon, decay and weight_decay must be non-negative")
        if not (0.0 <= group["beta_1"] < 1.0 and 0.0 <= group["beta_2"] < 1.0):
            raise ValueError("beta_1 and beta_2 must lie in [0, 1)")

    @staticmethod
    def _hyper(group):
        return tuple(float(group[k]) for k in ("lr", "beta_1", "beta_2", "epsilon", "decay", "weight_decay"))

    # ---- the scalars: one state block per device, a dictionary on the host for the tensor expressions -------------------------------
    def _block_keys(self):
        return [k for k in self.state if isinstance(k, str) and k.startswith(self._BLOCK)]

    @property
    def iterations(self):
        """Steps taken so far: the device's count where a device holds one (a copy to the host, i.e. a synchronisation)."""
        for k in self._block_keys():
            return nat.adam_state_read(self.state[k])[0]
        host = self.state.get(self._HOST)
        return host["iterations"] if host else self.__dict__.get("_start", 0)

    def _block(self, dev, start=None):
        key = self._BLOCK + str(dev)
        blk = self.state.get(key)
        if blk is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("Adam: the state block cannot be created inside a graph capture; take an eager step or call "
                                   "init_state() first")
            if start is None:
                start = self.iterations
            n = len(self.param_groups)
            blk = torch.zeros((nat.adam_state_bytes(n),), dtype=torch.uint8, device=dev)
            for gi, group in enumerate(self.param_groups):
                h = self._hyper(group)
                nat.adam_state_init(blk, n, gi, *h, iterations=start)
                self._seen[(key, gi)] = h
            self.state[key] = blk
        return blk

    def _rebuild_blocks(self):
        """New state blocks from `param_groups` at the step count the present ones (restored, or of another group count) hold."""
        keys = self._block_keys()
        self._start = self.iterations
        self._seen = {}
        for k in keys:
            del self.state[k]
        for k in keys:
            self._block(torch.device(k[len(self._BLOCK):]), self._start)

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        host = self.state.get(self._HOST)
        if host is not None:                                  # (state that belongs to no parameter is not copied by the framework)
            self.state[self._HOST] = {k: (list(v) if isinstance(v, list) else v) for k, v in host.items()}
        self._rebuild_blocks()

    def __setstate__(self, state):
        super().__setstate__(state)
        self._seen = {}                                       # what the blocks hold is read from `param_groups` again: see _push

    def add_param_group(self, param_group):
        if "_seen" in self.__dict__ and len(self.param_groups) >= nat.ADAM_MAX_GROUPS:
            raise ValueError("at most %d parameter groups (the device state block's size)" % nat.ADAM_MAX_GROUPS)
        super().add_param_group(param_group)
        if "_seen" in self.__dict__:                          # (not from the constructor)
            self._check(self.param_groups[-1])
            host = self.state.get(self._HOST)
            if host is not None:
                for name, beta in (("b1t", "beta_1"), ("b2t", "beta_2")):
                    host[name].append(self._product(self.param_groups[-1][beta], host["iterations"]))
            self._rebuild_blocks()

    @staticmethod
    def _product(beta, t):
        x = 1.0
        for _ in range(t):                                    # the tick's own sequence of float64 products, not pow()
            x = x * beta
        return x

    def _push(self, key, gi, group, blk):
        """The learning rate of `param_groups` into the block when it changed (eager steps only: a launch inside a capture would be
        replayed with the graph and undo every later `set_lr`)."""
        h = self._hyper(group)
        seen = self._seen.get((key, gi))
        if seen == h:
            return
        if seen is not None and seen[1:] != h[1:]:
            raise ValueError("Adam: only `lr` can change after the first step (group %d: %r -> %r)" % (gi, seen, h))
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("Adam: set the learning rate (set_lr, or an eager step) before the capture, not inside it")
        nat.optim_set_lr(blk, gi, h[0])
        self._seen[(key, gi)] = h

    def set_lr(self, lr, group=None):
        """A new base learning rate for one group (or all), on the current stream: between two replays of a captured step."""
        if not lr >= 0.0:
            raise ValueError("lr must be non-negative")
        for gi, g in enumerate(self.param_groups):
            if group is None or gi == group:
                g["lr"] = lr
                for key in self._block_keys():
                    nat.optim_set_lr(self.state[key], gi, lr)
                    self._seen[(key, gi)] = self._hyper(g)

    def _host_tick(self):
        """adam_tick_kernel on the host: float64 Python arithmetic, the same operations in the same order.  Returns lr_t per group."""
        host = self.state.get(self._HOST)
        if host is None:
            t = self.iterations
            host = self.state[self._HOST] = {"iterations": t, "b1t": [self._product(g["beta_1"], t) for g in self.param_groups],
                                             "b2t": [self._product(g["beta_2"], t) for g in self.param_groups]}
        host["iterations"] = t = host["iterations"] + 1
        lr_t = []
        for gi, g in enumerate(self.param_groups):
            b1t = host["b1t"][gi] = host["b1t"][gi] * float(g["beta_1"])
            b2t = host["b2t"][gi] = host["b2t"][gi] * float(g["beta_2"])
            lr = float(g["lr"])
            if g["decay"] > 0.0:
                lr = lr / (1.0 + float(g["decay"]) * float(t - 1))
            lr_t.append(lr * math.sqrt(1.0 - b2t) / (1.0 - b1t))
        return lr_t

    # ---- the step -------------------------------------------------------------------------------------------------------------------
    def _moments(self, p, amsgrad, capturing):
        st = self.state[p]
        for n in ("m", "v", "vhat") if amsgrad else ("m", "v"):
            if n not in st:
                if capturing:
                    raise RuntimeError("Adam: moment buffers cannot be created inside a graph capture; take an eager step or call "
                                       "init_state() first")
                st[n] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return st

    def _plan(self, gi, group):
        fused, rest = self._split(group, fusable=self._fused)
        ams = group["amsgrad"]
        capturing = torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()
        tables = []
        for dev, ps in fused.items():
            sts = [self._moments(p, ams, capturing) for p in ps]
            table = nat.adam_table([_flat(p) for p in ps], [_flat(p.grad) for p in ps], [_flat(st["m"]) for st in sts],
                                   [_flat(st["v"]) for st in sts], [_flat(st["vhat"]) for st in sts] if ams else None, dev)
            tables.append((table, tuple(ps), self._BLOCK + str(dev)))
        for p in rest:
            self._moments(p, ams, capturing and p.is_cuda)
        return tables, rest

    def init_state(self):
        """What the first step allocates -- moment buffers of the parameters that have a gradient now, the state block -- without a
        step: so that `step()` can be captured into a graph from step 1 on."""
        for gi, group in enumerate(self.param_groups):
            for _, _, key in self._planned(gi, group, (group["amsgrad"], self._fused))[0]:
                self._block(torch.device(key[len(self._BLOCK):]))

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        plans = [self._planned(gi, group, (group["amsgrad"], self._fused)) for gi, group in enumerate(self.param_groups)]
        # every group's learning rate first: the tick in front of the first update launch computes lr_t of ALL groups
        for gi, (tables, _) in enumerate(plans):
            for _, _, key in tables:
                self._push(key, gi, self.param_groups[gi], self._block(torch.device(key[len(self._BLOCK):])))
        ticked = set()
        for gi, (tables, _) in enumerate(plans):
            for table, ps, key in tables:
                nat.adam_step(table, self.state[key], gi, tick=key not in ticked)
                ticked.add(key)
                _bump_versions(ps)                                  # caches keyed on `_version` (the bf16 shadows) must see the update
        if any(rest for _, rest in plans):
            lr_ts = self._host_tick()
            for (_, rest), group, lr_t in zip(plans, self.param_groups, lr_ts):
                b1, b2, eps, wd = float(group["beta_1"]), float(group["beta_2"]), float(group["epsilon"]), float(group["weight_decay"])
                for p in rest:                                      # one rounding per operation, in the kernel's order: no `alpha=`
                    st = self.state[p]                              # forms (the framework evaluates those as a fused multiply-add)
                    g = p.grad.to_dense() if p.grad.is_sparse else p.grad
                    if wd != 0.0:
                        g = g + p * wd
                    m, v = st["m"], st["v"]
                    m.mul_(b1).add_(g * (1.0 - b1))
                    v.mul_(b2).add_((g * g) * (1.0 - b2))
                    den = v
                    if group["amsgrad"]:
                        den = torch.maximum(st["vhat"], v, out=st["vhat"])
                    # (the framework's vectorised CPU sqrt is one ulp off IEEE's on 0.7 % of values; the float64 one rounded to
                    #  float32 is the correctly rounded float32 root: 53 >= 2 * 24 + 2 bits, double rounding cannot show)
                    root = den.sqrt() if den.dtype == torch.float64 else den.double().sqrt().to(den.dtype)
                    p.sub_((m * lr_t) / (root + eps))
        return loss
