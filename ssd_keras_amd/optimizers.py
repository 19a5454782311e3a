"""The optimizers of the reference's training notebooks as torch optimizers whose step is ONE libssdhip launch over every parameter
instead of the framework's dozen multi-tensor launches (0.34 ms of an 11 ms SSD300 step, profiles/r05h_train_step_timeline.json).

`SGD` -- `keras.optimizers.SGD(lr=0.001, momentum=0.9, decay=0.0, nesterov=False)` under ssd300_training.ipynb's LearningRateScheduler
(ssd300_training.ipynb:169; csrc/ssdhip_optim.hip, sgd_tick_kernel / sgd_step_kernel).  Two update rules: `rule='torch'` (the default)
keeps torch.optim.SGD's momentum buffer (`buf = momentum * buf + g`, `p -= lr * buf`), `rule='keras'` Keras 2.x `SGD.get_updates`'
velocity (`v = momentum * v - lr * g`, `p += v`).  They are the same for a constant learning rate only: when the rate changes a velocity
keeps the rate it was built under, a momentum buffer is rescaled as a whole.  `nesterov` and Keras's time-based `decay`
(`lr = lr0 / (1 + decay * iterations)`, the count read before its increment) in both; `weight_decay` adds `weight_decay * p` to the
gradient first (Keras expresses the same thing as `kernel_regularizer=l2(5e-4)` on the loss, models/keras_ssd300.py:274: gradient
`2 * 5e-4 * W`).

`Adam` -- `keras.optimizers.Adam(lr=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-08, decay=0.0)`, the optimizer of every other notebook
(ssd7_training.ipynb:153; csrc/ssdhip_adam.hip).  Update rule: Keras 2.x `Adam.get_updates`, NOT torch.optim.Adam's --
`lr_t = lr * sqrt(1 - b2^t) / (1 - b1^t)`, `p -= lr_t * m / (sqrt(v) + epsilon)`: epsilon is added to the UNcorrected sqrt(v), 30 x the
effective epsilon of torch's rule at t = 1.  The step count, the running products b^t and every scalar of the update live in a state
block on the device that a tick kernel advances, so `step()` captured into a HIP graph replays with the bias correction of ITS step.

Both keep their scalars in such a state block per device (`iterations`, per group the base learning rate and what the update reads):
`set_lr` changes the learning rate between two replays of a captured step, `init_state()` allocates what a capture may not, and
`iterations` reads the device's count back.

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
    """What the one-launch optimizers share: which parameters are eligible, the cache of their pointer tables, and the scalars -- one
    state block per device that a tick kernel advances (`iterations`, per group the base learning rate and what the update reads),
    a dictionary on the host for the tensor expressions.  `lr` may change at any time -- through `param_groups` (a
    `torch.optim.lr_scheduler` does that; the next eager `step()` sends it to the device) or through `set_lr`, which is what a caller
    uses between two replays of a captured step; the other hyperparameters are fixed once the first step has been taken.

    A step inside `torch.cuda.graph` records the tick and the update launches only.  Nothing may be allocated there, so the state
    buffers and the state block must exist: take an eager step first, or call `init_state()` with the gradients in place.
    `iterations` reads the device's count back (a synchronisation: for logging and checkpoints).  A device's count advances with the
    update launches on that device and the host's with the tensor expressions: in an optimizer that mixes both, a step in which no
    parameter of a device has a gradient leaves that device's count one behind (the notebooks' models never do that).

    A subclass names its state (`_buffers`, `_BLOCK`, `_HOST`) and supplies `_check`, `_hyper` (lr first), `_tag`, `_plan`, the
    block's three native calls, `_launch` and `_expressions`."""

    _buffers = ()                                            # names of the per-parameter state tensors the kernel touches
    _BLOCK = None                                            # self.state[_BLOCK + device]: the device's state block, a uint8 tensor
    _HOST = None                                             # self.state[_HOST]: the same scalars for the tensor-expression path

    def __init__(self, params, defaults):
        self._check(defaults)
        super().__init__(params, defaults)
        self._tables, self._seen = {}, {}
        for group in self.param_groups:
            self._check(group)
        self._check_groups()

    def _check_groups(self):
        if len(self.param_groups) > nat.ADAM_MAX_GROUPS:
            raise ValueError("at most %d parameter groups (the device state block's size)" % nat.ADAM_MAX_GROUPS)

    # The device tables hold RAW pointers (parameter, gradient, state buffers): everything that can replace one of those tensors
    # drops them, and the per-step key below covers all their addresses as well (the key used to hold the gradients'
    # addresses only -- `load_state_dict` after a step replaced the momentum buffers, the kernel kept updating the freed ones).
    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._tables = {}
        host = self.state.get(self._HOST)
        if host is not None:                                  # (state that belongs to no parameter is not copied by the framework)
            self.state[self._HOST] = {k: (list(v) if isinstance(v, list) else v) for k, v in host.items()}
        self._rebuild_blocks()

    def __setstate__(self, state):
        super().__setstate__(state)
        self._tables = {}                                     # never pickled pointers: rebuilt on the next step
        self._seen = {}                                       # what the blocks hold is read from `param_groups` again: see _push

    def __getstate__(self):
        state = dict(super().__getstate__()) if hasattr(super(), "__getstate__") else dict(self.__dict__)
        state.pop("_tables", None)
        return state

    def add_param_group(self, param_group):
        late = "_seen" in self.__dict__                       # (not from the constructor)
        if late and len(self.param_groups) >= nat.ADAM_MAX_GROUPS:
            raise ValueError("at most %d parameter groups (the device state block's size)" % nat.ADAM_MAX_GROUPS)
        super().add_param_group(param_group)
        self._tables = {}
        if late:
            self._check(self.param_groups[-1])
            host = self.state.get(self._HOST)
            if host is not None:
                self._host_add_group(host, self.param_groups[-1])
            self._rebuild_blocks()

    def _host_add_group(self, host, group):
        pass

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
        11 ms), every microsecond of Python in it shows.  A table is (native table, its parameters, the block's key, the device)."""
        key = self._key(group)
        tabs = self.__dict__.setdefault("_tables", {})
        hit = tabs.get(gi)
        if hit is None or hit[0] != key or hit[1] != tag:
            plan = self._plan(gi, group)                     # (creates the missing state buffers: the key is taken again with them)
            hit = (self._key(group), tag) + plan
            tabs[gi] = hit
        return hit[2], hit[3]

    def _zeros(self, p, st, name, capturing):
        """The state buffer `name` of `p`, zeros in the parameter's layout when it does not exist yet."""
        if name not in st:
            if capturing:
                raise RuntimeError("%s: state buffers cannot be created inside a graph capture; take an eager step or call "
                                   "init_state() first" % type(self).__name__)
            st[name] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return st[name]

    # ---- the scalars: one state block per device, a dictionary on the host for the tensor expressions -------------------------------
    def _block_keys(self):
        return [k for k in self.state if isinstance(k, str) and k.startswith(self._BLOCK)]

    @property
    def iterations(self):
        """Steps taken so far: the device's count where a device holds one (a copy to the host, i.e. a synchronisation)."""
        for k in self._block_keys():
            return self._state_read(self.state[k])[0]
        host = self.state.get(self._HOST)
        return host["iterations"] if host else self.__dict__.get("_start", 0)

    def _block(self, dev, start=None):
        key = self._BLOCK + str(dev)
        blk = self.state.get(key)
        if blk is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("%s: the state block cannot be created inside a graph capture; take an eager step or call "
                                   "init_state() first" % type(self).__name__)
            if start is None:
                start = self.iterations
            n = len(self.param_groups)
            blk = torch.zeros((self._state_bytes(n),), dtype=torch.uint8, device=dev)
            for gi, group in enumerate(self.param_groups):
                h = self._hyper(group)
                self._state_init(blk, n, gi, h, start)
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

    def _push(self, key, gi, group, blk):
        """The learning rate of `param_groups` into the block when it changed (eager steps only: a launch inside a capture would be
        replayed with the graph and undo every later `set_lr`)."""
        h = self._hyper(group)
        seen = self._seen.get((key, gi))
        if seen == h:
            return
        name = type(self).__name__
        if seen is not None and seen[1:] != h[1:]:
            raise ValueError("%s: only `lr` can change after the first step (group %d: %r -> %r)" % (name, gi, seen, h))
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("%s: set the learning rate (set_lr, or an eager step) before the capture, not inside it" % name)
        self._set_lr(blk, gi, h[0])
        self._seen[(key, gi)] = h

    def set_lr(self, lr, group=None):
        """A new base learning rate for one group (or all), on the current stream: between two replays of a captured step."""
        if not lr >= 0.0:
            raise ValueError("lr must be non-negative")
        for gi, g in enumerate(self.param_groups):
            if group is None or gi == group:
                g["lr"] = lr
                for key in self._block_keys():
                    self._set_lr(self.state[key], gi, lr)
                    self._seen[(key, gi)] = self._hyper(g)

    # ---- the step -------------------------------------------------------------------------------------------------------------------
    def init_state(self):
        """What the first step allocates -- state buffers of the parameters that have a gradient now, the state block -- without a
        step: so that `step()` can be captured into a graph from step 1 on."""
        for gi, group in enumerate(self.param_groups):
            for _, _, _, dev in self._planned(gi, group, self._tag(group))[0]:
                self._block(dev)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        groups = self.param_groups
        plans = [self._planned(gi, group, self._tag(group)) for gi, group in enumerate(groups)]
        # every group's learning rate first: the tick in front of the first update launch computes lr_t of ALL groups
        for gi, (tables, _) in enumerate(plans):
            for _, _, key, dev in tables:
                self._push(key, gi, groups[gi], self._block(dev))
        ticked = set()
        for gi, (tables, _) in enumerate(plans):
            for table, ps, key, _ in tables:
                self._launch(table, self.state[key], gi, groups[gi], key not in ticked)
                ticked.add(key)
                _bump_versions(ps)                                  # caches keyed on `_version` (the bf16 shadows) must see the update
        if any(rest for _, rest in plans):
            self._expressions(plans, self._host_tick())
        return loss


_flat = lambda t: t.detach().as_strided((t.numel(),), (1,))


class SGD(_OneLaunchOptimizer):
    """keras.optimizers.SGD with Keras's parameter names (`decay`, `nesterov`) beside torch's (`weight_decay`); `rule` picks the state
    it keeps: 'torch' the momentum buffer of torch.optim.SGD (state key "momentum_buffer"), 'keras' the velocity of Keras 2.x
    `SGD.get_updates` (state key "velocity") -- see the module docstring for where they part.  Learning rate, captures, `init_state`
    and `iterations` as described in `_OneLaunchOptimizer`.  Parameters of a group with momentum 0 keep no state and go through the
    tensor expressions."""

    _buffers = ("momentum_buffer", "velocity")
    _BLOCK = "sgd_state:"
    _HOST = "sgd_host"
    _BUFFER = {"torch": "momentum_buffer", "keras": "velocity"}

    def __init__(self, params, lr=0.01, momentum=0.0, weight_decay=0.0, decay=0.0, nesterov=False, rule="torch"):
        super().__init__(params, dict(lr=lr, momentum=momentum, weight_decay=weight_decay, decay=decay, nesterov=bool(nesterov), rule=rule))

    @staticmethod
    def _check(group):
        if not (group["lr"] >= 0.0 and group["momentum"] >= 0.0 and group["weight_decay"] >= 0.0 and group["decay"] >= 0.0):
            raise ValueError("lr, momentum, weight_decay and decay must be non-negative")
        if group["rule"] not in nat.SGD_RULES:
            raise ValueError("rule must be 'torch' or 'keras' (got %r)" % (group["rule"],))
        if group["nesterov"] and group["momentum"] == 0.0:
            raise ValueError("nesterov needs a momentum")

    @staticmethod
    def _hyper(group):
        return (float(group["lr"]), float(group["momentum"]), float(group["decay"]), float(group["weight_decay"]), bool(group["nesterov"]),
                group["rule"])

    @staticmethod
    def _tag(group):
        return (group["momentum"] != 0.0, group["rule"])

    _state_bytes = staticmethod(nat.sgd_state_bytes)
    _state_read = staticmethod(nat.sgd_state_read)
    _set_lr = staticmethod(nat.sgd_set_lr)

    @staticmethod
    def _state_init(blk, n, gi, h, start):
        nat.sgd_state_init(blk, n, gi, h[0], h[1], h[2], h[3], iterations=start)

    def _host_tick(self):
        """sgd_tick_kernel on the host: float64 Python arithmetic, the same operations in the same order.  Returns lr_t per group."""
        host = self.state.get(self._HOST)
        if host is None:
            host = self.state[self._HOST] = {"iterations": self.iterations}
        host["iterations"] = t = host["iterations"] + 1
        lr_t = []
        for g in self.param_groups:
            lr = float(g["lr"])
            if g["decay"] > 0.0:
                lr = lr / (1.0 + float(g["decay"]) * float(t - 1))
            lr_t.append(lr)
        return lr_t

    def _plan(self, gi, group):
        fused, rest = self._split(group, fusable=group["momentum"] != 0.0)
        name = self._BUFFER[group["rule"]]
        capturing = torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()
        tables = []
        for dev, ps in fused.items():
            bufs = [self._zeros(p, self.state[p], name, capturing) for p in ps]   # zeros: torch's first buf = grad, Keras's v = 0
            table = nat.sgd_table([_flat(p) for p in ps], [_flat(p.grad) for p in ps], [_flat(b) for b in bufs], dev)
            tables.append((table, tuple(ps), self._BLOCK + str(dev), dev))
        if group["momentum"] != 0.0:
            for p in rest:
                self._zeros(p, self.state[p], name, capturing and p.is_cuda)
        return tables, rest

    @staticmethod
    def _launch(table, blk, gi, group, tick):
        nat.sgd_step(table, blk, gi, nat.SGD_RULES[group["rule"]], group["nesterov"], tick)

    def _expressions(self, plans, lr_ts):
        for (_, rest), group, lr in zip(plans, self.param_groups, lr_ts):
            mom, wd, nesterov = float(group["momentum"]), float(group["weight_decay"]), group["nesterov"]
            keras, name = group["rule"] == "keras", self._BUFFER[group["rule"]]
            for p in rest:                                          # one rounding per operation, in the kernel's order: no `alpha=`
                g = p.grad.to_dense() if p.grad.is_sparse else p.grad   # forms (the framework evaluates those as a fused multiply-add)
                if wd != 0.0:
                    g = g + p * wd
                if mom == 0.0:                                      # no state: both rules are p - lr g
                    p.sub_(g * lr)
                elif keras:
                    v, lg = self.state[p][name], g * lr
                    v.mul_(mom).sub_(lg)
                    if nesterov:
                        p.add_(v * mom).sub_(lg)
                    else:
                        p.add_(v)
                else:
                    buf = self.state[p][name]
                    buf.mul_(mom).add_(g)
                    p.sub_((g + buf * mom) * lr if nesterov else buf * lr)


class Adam(_OneLaunchOptimizer):
    """keras.optimizers.Adam with Keras's parameter names and defaults (`epsilon=None` is K.epsilon() = 1e-7; the notebooks pass 1e-08);
    `weight_decay` per group as in `SGD` (Keras's l2 kernel regulariser).  Learning rate, captures, `init_state` and `iterations` as
    described in `_OneLaunchOptimizer`.
    `_fused = False` on an instance is a TEST HOOK: every parameter then goes through the tensor expressions, which is what the tests
    compare the kernel with."""

    _buffers = ("m", "v", "vhat")
    _BLOCK = "adam_state:"
    _HOST = "adam_host"
    _fused = True

    def __init__(self, params, lr=0.001, beta_1=0.9, beta_2=0.999, epsilon=None, decay=0.0, amsgrad=False, weight_decay=0.0):
        if epsilon is None:
            epsilon = 1e-7
        super().__init__(params, dict(lr=lr, beta_1=beta_1, beta_2=beta_2, epsilon=epsilon, decay=decay, amsgrad=bool(amsgrad),
                                      weight_decay=weight_decay))

    @staticmethod
    def _check(group):
        if not (group["lr"] >= 0.0 and group["epsilon"] >= 0.0 and group["decay"] >= 0.0 and group["weight_decay"] >= 0.0):
            raise ValueError("lr, epsilon, decay and weight_decay must be non-negative")
        if not (0.0 <= group["beta_1"] < 1.0 and 0.0 <= group["beta_2"] < 1.0):
            raise ValueError("beta_1 and beta_2 must lie in [0, 1)")

    @staticmethod
    def _hyper(group):
        return tuple(float(group[k]) for k in ("lr", "beta_1", "beta_2", "epsilon", "decay", "weight_decay"))

    def _tag(self, group):
        return (group["amsgrad"], self._fused)

    _state_bytes = staticmethod(nat.adam_state_bytes)
    _state_read = staticmethod(nat.adam_state_read)
    _set_lr = staticmethod(nat.optim_set_lr)

    @staticmethod
    def _state_init(blk, n, gi, h, start):
        nat.adam_state_init(blk, n, gi, *h, iterations=start)

    def _host_add_group(self, host, group):
        for name, beta in (("b1t", "beta_1"), ("b2t", "beta_2")):
            host[name].append(self._product(group[beta], host["iterations"]))

    @staticmethod
    def _product(beta, t):
        x = 1.0
        for _ in range(t):                                    # the tick's own sequence of float64 products, not pow()
            x = x * beta
        return x

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

    def _moments(self, p, amsgrad, capturing):
        st = self.state[p]
        for n in ("m", "v", "vhat") if amsgrad else ("m", "v"):
            self._zeros(p, st, n, capturing)
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
            tables.append((table, tuple(ps), self._BLOCK + str(dev), dev))
        for p in rest:
            self._moments(p, ams, capturing and p.is_cuda)
        return tables, rest

    @staticmethod
    def _launch(table, blk, gi, group, tick):
        nat.adam_step(table, blk, gi, tick=tick)

    def _expressions(self, plans, lr_ts):
        for (_, rest), group, lr_t in zip(plans, self.param_groups, lr_ts):
            b1, b2, eps, wd = float(group["beta_1"]), float(group["beta_2"]), float(group["epsilon"]), float(group["weight_decay"])
            for p in rest:                                          # one rounding per operation, in the kernel's order: no `alpha=`
                st = self.state[p]                                  # forms (the framework evaluates those as a fused multiply-add)
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
