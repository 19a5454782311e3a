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

`master_weights=True` (per group) is how a bf16 model is trained: the optimizer keeps a float32 master copy of every bf16 parameter
(`state[p]["master"]`, the moments float32 beside it), runs the float32 rule on the master with the bf16 gradient widened exactly, and
writes the parameter as the master rounded to nearest even.  Without it a bf16 parameter is updated in bf16, where an update below
half an ulp of the weight -- 2^-9 of its magnitude -- rounds to nothing, step after step.

In both, float32 parameters on a GPU with gradients of their own memory layout take the fused launch, and so do bf16 parameters with
bf16 gradients under `master_weights` (a launch of their own: ssdhip_adam_step_bf16 / ssdhip_sgd_step_bf16); anything else (CPU
tensors, other dtypes, bf16 without masters, SGD with momentum 0) the plain tensor expressions of the same rule.  All four launches
are ONE update body and one host launcher (csrc/ssdhip_optim_step.h) with the optimizer's rule in it, planned in one place here.

`clipnorm=` / `clipvalue=` -- the two keywords every keras.optimizers.Optimizer takes, as Keras 2.2.4's `Optimizer.get_gradients` /
`clip_norm` define them (restated from its source in tests/np_clip.py: there is no Keras where this runs): ONE norm over all
parameters of the optimizer, `g * clipnorm / norm` when `norm >= clipnorm`, then the clamp to `[-clipvalue, clipvalue]`.  `g` is the
gradient of the PENALISED loss, here `g + weight_decay * w` (w the parameter, or its master), which `torch.nn.utils.clip_grad_norm_`
between `backward()` and `step()` never sees -- and that call could not be captured.  The norm is taken on the device over the step's
own tensor tables (ssdhip_grad_sumsq_partials, one launch per table, in the written-down order of additions of
ssdhip_sumsq_partials), ssdhip_clip_finish turns it into a scale in a clip state block, and the clipped forms of the four step
launches apply it: a captured step replays with the norm of ITS gradients.  A NaN norm clips nothing and an infinite one scales by 0,
as in Keras.  `skip_nonfinite=True` is this package's own (as `rule='torch'` is): a step whose sum of squares is not finite does
nothing -- no parameter, master or buffer is written, `iterations` and Adam's products stay --, and is counted; it may be given
alone.  `grad_norm` reads the last norm back, `clip_stats` the counters {'steps', 'clipped', 'skipped'}.  The three are
optimizer-wide; with any of them set every parameter that has a gradient must take the fused launch, on one device -- the tensor
expressions (SGD with momentum 0, bf16 without masters, CPU tensors, other dtypes) do not clip and `step()` refuses them with a
ValueError before anything is launched.  Without the keywords no clip block exists and the step is the one described above."""
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


class _MasterWeightsOption(type):
    """`master_weights=` at construction: `SGD(params, ..., master_weights=True)`.  Why a metaclass and not an ordinary keyword of
    the two `__init__`: tests/test_sgd_cpu.py and tests/test_optim_cpu.py pin the exact parameter lists of `SGD.__init__` and
    `Adam.__init__`, so the keyword is taken here, in front of `__init__`, and handed to `_OneLaunchOptimizer.__init__` as a default of
    the parameter groups.  The price: `inspect.signature(SGD)` and `help(SGD)` show `(*args, master_weights=False, **kwargs)` -- the
    Keras parameters are on `SGD.__init__` --, and a subclass cannot forward the option through `super().__init__`: it passes it where
    it constructs (`Sub(..., master_weights=True)`), or sets `group["master_weights"]` before the first step.  Once those two lists may
    grow, this class goes and `master_weights=False` becomes a keyword-only parameter of the two constructors.
    `clipnorm=`, `clipvalue=` and `skip_nonfinite=` (gradient clipping, `_OneLaunchOptimizer`) are taken the same way."""

    def __call__(cls, *args, master_weights=False, clipnorm=None, clipvalue=None, skip_nonfinite=False, **kwargs):
        self = cls.__new__(cls)
        self._master_weights_default = bool(master_weights)
        self._clip_default = dict(clipnorm=clipnorm, clipvalue=clipvalue, skip_nonfinite=bool(skip_nonfinite))   # (the same route)
        self.__init__(*args, **kwargs)
        return self


class _OneLaunchOptimizer(torch.optim.Optimizer, metaclass=_MasterWeightsOption):
    """What the one-launch optimizers share: which parameters are eligible, the cache of their pointer tables, and the scalars -- one
    state block per device that a tick kernel advances (`iterations`, per group the base learning rate and what the update reads),
    a dictionary on the host for the tensor expressions.  `lr` may change at any time -- through `param_groups` (a
    `torch.optim.lr_scheduler` does that; the next eager `step()` sends it to the device) or through `set_lr`, which is what a caller
    uses between two replays of a captured step; the other hyperparameters are fixed once the first step has been taken.

    A step inside `torch.cuda.graph` records the tick and the update launches only.  Nothing may be allocated there, so the state
    buffers (the masters among them) and the state block must exist: take an eager step first, or call `init_state()` with the
    gradients in place.
    `iterations` reads the device's count back (a synchronisation: for logging and checkpoints).  A device's count advances with the
    update launches on that device and the host's with the tensor expressions: in an optimizer that mixes both, a step in which no
    parameter of a device has a gradient leaves that device's count one behind (the notebooks' models never do that).

    Masters (`master_weights`): a master is made from its parameter once (`p.float()`, exact) and is the truth from then on.  The
    optimizer remembers each parameter's `_version` after its own update; an eager `step()` that finds another one (the model loaded a
    checkpoint, somebody wrote the weights in place) takes the master from the parameter again before it updates.  A captured step
    cannot (the copy would replay every time): it raises, and `sync_masters()` is the call to make -- before the capture, or between
    two replays after loading weights.  A master's creation (the first step, `init_state()`) remembers the version too, so weights
    loaded after `init_state()` are found.  No remembered version (a master that came with a restored or unpickled optimizer) means
    the master is trusted.

    A subclass names its state (`_buffers`, `_BLOCK`, `_HOST`), says which buffers a group's parameters have (`_group_buffers`) and
    whether it can take the fused launch (`_fusable`), and supplies `_check`, `_hyper` (lr first), `_tag`, the block's three native
    calls, `_table`, `_launch` and `_expressions`.

    Clipping (`clipnorm`, `clipvalue`, `skip_nonfinite`; the module docstring): the settings live in the groups' defaults, so
    `state_dict`, `load_state_dict` and pickling carry them; the clip state block is `state["clip_state:" + device]`, the partials
    buffer (one float32 per 8192-element chunk of every parameter) an attribute that is never saved; both are made by the first eager
    step or by `init_state()`, never inside a capture.  The block sits in `state` beside the optimizer's state block, so
    `state_dict()` writes its 64 bytes; `load_state_dict` ignores them and a restored optimizer starts its counters again from the
    settings in the groups.  On a step that `skip_nonfinite` skips the host cannot know (it reads nothing back): the parameters'
    `_version` is bumped as on every step, and caches keyed on it refresh from unchanged weights."""

    _buffers = ()                                            # names of the per-parameter state tensors the kernel touches
    _BLOCK = None                                            # self.state[_BLOCK + device]: the device's state block, a uint8 tensor
    _HOST = None                                             # self.state[_HOST]: the same scalars for the tensor-expression path
    _FUSED_NEEDS = ""                                        # what else the fused launch asks of a group, for _clip_refuse's message

    def __init__(self, params, defaults):
        defaults = dict(defaults, master_weights=self.__dict__.pop("_master_weights_default", False),   # (_MasterWeightsOption)
                        **self.__dict__.pop("_clip_default", _NO_CLIP))
        self._check(defaults)
        super().__init__(params, defaults)
        self._tables, self._seen, self._versions, self._mastering = {}, {}, {}, {}
        self._clip_partials, self._clip_set = {}, {}
        for group in self.param_groups:
            self._check(group)
        self._check_groups()

    def _check_groups(self):
        if len(self.param_groups) > nat.ADAM_MAX_GROUPS:
            raise ValueError("at most %d parameter groups (the device state block's size)" % nat.ADAM_MAX_GROUPS)
        self._clip()

    def _clip(self):
        """(clipnorm, clipvalue, skip_nonfinite) of the optimizer, 0.0 for a bound that is off, or None when none of the three is set:
        they are optimizer-wide (ONE norm over every parameter), so groups that disagree raise, and so does a negative bound."""
        name, found = type(self).__name__, None
        for gi, group in enumerate(self.param_groups):
            cn, cv = group.get("clipnorm"), group.get("clipvalue")
            for what, x in (("clipnorm", cn), ("clipvalue", cv)):
                if x is not None and not float(x) >= 0.0:
                    raise ValueError("%s: %s must be non-negative (group %d: %r)" % (name, what, gi, x))
            here = (float(cn or 0.0), float(cv or 0.0), bool(group.get("skip_nonfinite", False)))
            if found is not None and here != found:
                raise ValueError("%s: clipnorm, clipvalue and skip_nonfinite are optimizer-wide (group 0: %r, group %d: %r)"
                                 % (name, found, gi, here))
            found = here
        return found if found and (found[0] > 0.0 or found[1] > 0.0 or found[2]) else None

    # The device tables hold RAW pointers (parameter, gradient, state buffers): everything that can replace one of those tensors
    # drops them, and the per-step key below covers all their addresses as well (the key used to hold the gradients'
    # addresses only -- `load_state_dict` after a step replaced the momentum buffers, the kernel kept updating the freed ones).
    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._tables, self._versions, self._mastering = {}, {}, {}
        for group in self.param_groups:                       # (a checkpoint from before the options existed)
            group.setdefault("master_weights", False)
            for k, v in _NO_CLIP.items():
                group.setdefault(k, v)
        for k in [k for k in self.state if isinstance(k, str) and k.startswith(_CLIP_BLOCK)]:
            del self.state[k]                                 # (made again, counters at zero, from the settings just loaded)
        self._clip_partials = {}
        self._clip()
        # (the framework casts every floating-point state tensor to its parameter's dtype: the float32 state of a bf16 parameter is
        #  taken from the checkpoint again, as it was saved)
        saved, ids = state_dict["state"], [i for g in state_dict["param_groups"] for i in g["params"]]
        for i, p in zip(ids, (p for g in self.param_groups for p in g["params"])):
            if "master" in saved.get(i, ()):
                for name, t in saved[i].items():
                    if torch.is_tensor(t) and t.is_floating_point() and t.dtype != p.dtype:
                        self.state[p][name] = t.detach().to(device=p.device, copy=True)
        host = self.state.get(self._HOST)
        if host is not None:                                  # (state that belongs to no parameter is not copied by the framework)
            self.state[self._HOST] = {k: (list(v) if isinstance(v, list) else v) for k, v in host.items()}
        self._rebuild_blocks()

    def __setstate__(self, state):
        super().__setstate__(state)
        self._tables = {}                                     # never pickled pointers: rebuilt on the next step
        self._seen = {}                                       # what the blocks hold is read from `param_groups` again: see _push
        self._versions, self._mastering = {}, {}              # (keyed by the parameters of the optimizer this was copied from)
        for group in self.param_groups:
            group.setdefault("master_weights", False)
            for k, v in _NO_CLIP.items():
                group.setdefault(k, v)
        self._clip_partials, self._clip_set = {}, {}

    def __getstate__(self):
        state = dict(super().__getstate__()) if hasattr(super(), "__getstate__") else dict(self.__dict__)
        for name in ("_tables", "_versions", "_mastering", "_clip_partials", "_clip_set"):
            state.pop(name, None)
        return state

    def add_param_group(self, param_group):
        late = "_seen" in self.__dict__                       # (not from the constructor)
        if late and len(self.param_groups) >= nat.ADAM_MAX_GROUPS:
            raise ValueError("at most %d parameter groups (the device state block's size)" % nat.ADAM_MAX_GROUPS)
        super().add_param_group(param_group)
        self._tables = {}
        if late:
            self._check(self.param_groups[-1])
            self._clip()
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

    @staticmethod
    def _mastered(group, p):
        """`p` is updated through a float32 master: a bf16 parameter of a group with `master_weights`."""
        return group["master_weights"] and p.dtype == torch.bfloat16

    def _split(self, group, fusable=True):
        """The parameters of a group that have a gradient: {(device, bf16 with a master): those that take a fused launch}, [the
        others]."""
        fused, rest = {}, []
        for p in group["params"]:
            g = p.grad
            if g is None:
                continue
            bf16 = self._mastered(group, p)
            ok = (fusable and p.is_cuda and (bf16 or p.dtype == torch.float32) and g.dtype == p.dtype and not g.is_sparse
                  and self._dense(p) and self._same_order(g, p) and p.data_ptr() % 16 == 0 and g.data_ptr() % 16 == 0)
            if ok:
                fused.setdefault((p.device, bf16), []).append(p)
            else:
                rest.append(p)
        return fused, rest

    def _key(self, group):
        """Which parameters have a gradient, and where the tensors the kernel touches live."""
        state, names = self.state, self._buffers + ("master",)
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
        11 ms), every microsecond of Python in it shows.  A table is (native table, its parameters, the block's key, the device,
        bf16 parameters with masters)."""
        key = self._key(group)
        tabs = self.__dict__.setdefault("_tables", {})
        hit = tabs.get(gi)
        if hit is None or hit[0] != key or hit[1] != tag:
            plan = self._plan(gi, group)                     # (creates the missing state buffers: the key is taken again with them)
            hit = (self._key(group), tag) + plan
            tabs[gi] = hit
        return hit[2], hit[3]

    def _plan(self, gi, group):
        """Per (device, bf16 with a master) one native table over the group's parameters that take the fused launch -- columns:
        parameter, gradient, the master if there is one, `_group_buffers(group)` -- and the rest for the tensor expressions; creates
        the masters and the state buffers that are missing (zeros: torch's first buf = grad, Keras's v = 0, Adam's moments)."""
        fused, rest = self._split(group, fusable=self._fusable(group))
        names = self._group_buffers(group)
        capturing = torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()

        def state(p, master, capturing):                     # (the master first: the buffers are made in its dtype)
            return ([self._master(p, self.state[p], capturing)] if master else []) + [self._zeros(p, self.state[p], n, capturing) for n in names]

        tables = []
        for (dev, bf16), ps in fused.items():
            rows = [[p, p.grad] + state(p, bf16, capturing) for p in ps]
            tables.append((self._table([[_flat(t) for t in col] for col in zip(*rows)], dev, bf16), tuple(ps), self._BLOCK + str(dev), dev, bf16))
        for p in rest:
            state(p, self._mastered(group, p), capturing and p.is_cuda)
        return tables, rest

    def _zeros(self, p, st, name, capturing):
        """The state buffer `name` of `p`, zeros in the parameter's layout (float32 beside a master) when it does not exist yet."""
        if name not in st:
            if capturing:
                raise RuntimeError("%s: state buffers cannot be created inside a graph capture; take an eager step or call "
                                   "init_state() first" % type(self).__name__)
            st[name] = torch.zeros_like(st.get("master", p), memory_format=torch.preserve_format)
        return st[name]

    def _master(self, p, st, capturing):
        """The float32 master of a bf16 parameter, in the parameter's layout: `p.float()` (exact) when it does not exist yet."""
        if "master" not in st:
            if capturing:
                raise RuntimeError("%s: master weights cannot be created inside a graph capture; take an eager step or call "
                                   "init_state() first" % type(self).__name__)
            st["master"] = p.detach().to(torch.float32, memory_format=torch.preserve_format, copy=True)
            self._versions[p] = p._version                        # init_state(), THEN the model loads weights: found, not trusted
            for name in self._buffers:                            # moments of a checkpoint saved without masters: widened (exact)
                if name in st and st[name].dtype != torch.float32:
                    st[name] = st[name].to(torch.float32, memory_format=torch.preserve_format)
        return st["master"]

    def _masters(self, plans):
        """Per group, the parameters of this step that have a master."""
        out = []
        for (tables, rest), group in zip(plans, self.param_groups):
            ps = [p for _, tps, _, _, bf16 in tables if bf16 for p in tps]
            if group["master_weights"]:
                ps += [p for p in rest if p.dtype == torch.bfloat16]
            out.append(ps)
        return out

    def sync_masters(self):
        """Every master from its parameter again (exact), on the current stream: after the model's weights were written by somebody
        else -- `load_state_dict`, `load_keras_weights`, an in-place edit -- and the next step is a captured one or a replay."""
        with torch.no_grad():
            for group in self.param_groups:
                for p in group["params"]:
                    st = self.state[p] if p in self.state else ()
                    if "master" in st:
                        st["master"].copy_(p)
                        self._versions[p] = p._version

    def mark_replayed(self):
        """After replays of a captured `step()`, which run no Python: the host's share of an eager step -- the `_version` of every
        parameter that has a gradient bumped once (caches keyed on it, the models' derived tensors among them, must see the update)
        and, for the parameters with a master, remembered as this optimizer's own write."""
        ps = [p for group in self.param_groups for p in group["params"] if p.grad is not None]
        if ps:
            _bump_versions(ps)
        for p in ps:
            if p in self._versions:
                self._versions[p] = p._version

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
        """What the first step allocates -- state buffers of the parameters that have a gradient now, the state block, with clipping
        the clip block and the partials buffer -- without a step: so that `step()` can be captured into a graph from step 1 on."""
        clip = self._clip()
        if clip is not None:
            self._clip_refuse()
        plans = [self._planned(gi, group, self._tag(group)) for gi, group in enumerate(self.param_groups)]
        for tables, _ in plans:
            for _, _, _, dev, _ in tables:
                self._block(dev)
        if clip is not None:
            self._clip_buffers(plans, clip)

    # ---- gradient clipping: Keras's clipnorm / clipvalue, and skip_nonfinite ----------------------------------------------------------
    def _clip_refuse(self):
        """With clipping every parameter that has a gradient takes the fused launch, on one device (the norm is ONE launch sequence on
        one stream): anything else is refused here, BEFORE anything is allocated or launched, naming the first such parameter.
        Decided anew at every step (`_split`, cheap beside `_planned`): a group's momentum or `master_weights` may have changed."""
        name, first = type(self).__name__, None
        for gi, group in enumerate(self.param_groups):
            fused, rest = self._split(group, fusable=self._fusable(group))
            bad = rest[0] if rest else None
            for (dev, _), ps in fused.items():
                first = first or dev
                if dev != first and bad is None:
                    bad = ps[0]
            if bad is not None:
                i = [id(p) for p in group["params"]].index(id(bad))
                raise ValueError(
                    "%s: clipnorm / clipvalue / skip_nonfinite need every parameter on the fused launch, on one device -- float32 (or bf16 "
                    "with master_weights) on a GPU, a dense gradient of its dtype and layout%s; parameter %d of group %d (shape %s, %s, %s) "
                    "is not" % (name, self._FUSED_NEEDS, i, gi, tuple(bad.shape), bad.dtype, bad.device))

    def _clip_buffers(self, plans, clip):
        """(clip block, partials buffer, number of partials) of this step's tables; creates what is missing (never inside a capture)
        and sends changed settings to the block (eager steps only).  The partials buffer is sized once for EVERY parameter of the
        optimizer, with a gradient or not, so that it never moves under a captured step when further parameters get gradients; only
        `add_param_group` can outgrow it, and that invalidates earlier captures anyway (it drops the tables)."""
        tables = [t for ts, _ in plans for t in ts]
        if not tables:
            return None, None, 0
        dev = tables[0][3]
        chunks = sum(nat.sumsq_chunks(p.numel() for p in ps) for _, ps, _, _, _ in tables)
        key = _CLIP_BLOCK + str(dev)
        blk, partials = self.state.get(key), self._clip_partials.get(dev)
        capturing = torch.cuda.is_current_stream_capturing()
        if capturing and (blk is None or partials is None or partials.numel() < chunks or self._clip_set.get(key) != clip):
            raise RuntimeError("%s: the clip block and its partials cannot be created or changed inside a graph capture; take an eager "
                               "step or call init_state() first" % type(self).__name__)
        if blk is None:
            blk = self.state[key] = torch.zeros((nat.clip_state_bytes(),), dtype=torch.uint8, device=dev)
            self._clip_set.pop(key, None)
        if self._clip_set.get(key) != clip:
            if key in self._clip_set:
                raise ValueError("%s: clipnorm, clipvalue and skip_nonfinite cannot change after the first step" % type(self).__name__)
            nat.clip_state_init(blk, *clip)
            self._clip_set[key] = clip
        if partials is None or partials.numel() < chunks:
            most = sum(nat.sumsq_chunks(p.numel() for p in group["params"]) for group in self.param_groups)
            partials = self._clip_partials[dev] = torch.empty((most,), dtype=torch.float32, device=dev)
        return blk, partials, chunks

    def _clip_read(self):
        for k in self.state:
            if isinstance(k, str) and k.startswith(_CLIP_BLOCK):
                return nat.clip_state_read(self.state[k])
        return None

    @property
    def grad_norm(self):
        """The global norm of the last step's gradients (of the penalised loss), as the device computed it: a read-back like
        `iterations`.  None before the first step of an optimizer that clips, and always in one that does not."""
        st = self._clip_read()
        return float(st["norm"]) if st is not None and st["steps"] > 0 else None

    @property
    def clip_stats(self):
        """{'steps', 'clipped', 'skipped'}: steps taken with clipping on, of them scaled down by `clipnorm`, of them skipped by
        `skip_nonfinite` (a read-back; the counters start again with a restored optimizer)."""
        st = self._clip_read()
        return {k: int(st[k]) if st is not None else 0 for k in ("steps", "clipped", "skipped")}

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        groups = self.param_groups
        clip = self._clip()
        if clip is not None:
            self._clip_refuse()
        for gi, group in enumerate(groups):
            if self._mastering.setdefault(gi, group["master_weights"]) != group["master_weights"]:
                raise ValueError("%s: `master_weights` cannot change after the first step (group %d)" % (type(self).__name__, gi))
        plans = [self._planned(gi, group, self._tag(group)) for gi, group in enumerate(groups)]
        masters = self._masters(plans)
        versions = self._versions
        for ps in masters:                                          # somebody else wrote the parameter: it is the truth now
            for p in ps:
                if versions.get(p, p._version) != p._version:
                    if p.is_cuda and torch.cuda.is_current_stream_capturing():
                        raise RuntimeError("%s: a parameter changed behind its master weights; call sync_masters() before the capture "
                                           "(a copy recorded into the graph would replay with every step)" % type(self).__name__)
                    self.state[p]["master"].copy_(p)
        # every group's learning rate first: the tick in front of the first update launch computes lr_t of ALL groups
        for gi, (tables, _) in enumerate(plans):
            for _, _, key, dev, _ in tables:
                self._push(key, gi, groups[gi], self._block(dev))
        cblk = None
        if clip is not None:                                       # the norm of g + weight_decay * w over every table, then the scale
            cblk, partials, chunks = self._clip_buffers(plans, clip)
            at = 0
            for gi, (tables, _) in enumerate(plans):
                for table, ps, _, _, bf16 in tables:
                    n = nat.sumsq_chunks(p.numel() for p in ps)
                    nat.optim_grad_sumsq_partials(table, bf16, groups[gi]["weight_decay"], partials[at:at + n])
                    at += n
            if cblk is not None:
                nat.clip_finish(cblk, partials[:chunks])
        ticked = set()
        for gi, (tables, _) in enumerate(plans):
            for table, ps, key, _, bf16 in tables:
                self._launch(table, self.state[key], gi, groups[gi], key not in ticked, bf16, cblk)
                ticked.add(key)
                _bump_versions(ps)                                  # caches keyed on `_version` (the bf16 shadows) must see the update
        if any(rest for _, rest in plans):
            self._expressions(plans, self._host_tick())
        for ps in masters:
            for p in ps:
                versions[p] = p._version
        return loss


_flat = lambda t: t.detach().as_strided((t.numel(),), (1,))
_NO_CLIP = dict(clipnorm=None, clipvalue=None, skip_nonfinite=False)   # the groups' defaults: no clipping
_CLIP_BLOCK = "clip_state:"                                  # self.state[_CLIP_BLOCK + device]: the device's clip state block


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
    _FUSED_NEEDS = ", a non-zero momentum"

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
        return (group["momentum"] != 0.0, group["rule"], group["master_weights"])

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

    def _group_buffers(self, group):                         # (momentum 0 keeps no state: both rules are p - lr g)
        return (self._BUFFER[group["rule"]],) if group["momentum"] != 0.0 else ()

    _fusable = staticmethod(lambda group: group["momentum"] != 0.0)

    @staticmethod
    def _table(cols, dev, bf16):
        return (nat.sgd_table_bf16 if bf16 else nat.sgd_table)(*cols, dev)

    @staticmethod
    def _launch(table, blk, gi, group, tick, bf16, clip=None):
        (nat.sgd_step_bf16 if bf16 else nat.sgd_step)(table, blk, gi, nat.SGD_RULES[group["rule"]], group["nesterov"], tick, clip)

    def _expressions(self, plans, lr_ts):
        for (_, rest), group, lr in zip(plans, self.param_groups, lr_ts):
            mom, wd, nesterov = float(group["momentum"]), float(group["weight_decay"]), group["nesterov"]
            keras, name = group["rule"] == "keras", self._BUFFER[group["rule"]]
            for p in rest:                                          # one rounding per operation, in the kernel's order: no `alpha=`
                g = p.grad.to_dense() if p.grad.is_sparse else p.grad   # forms (the framework evaluates those as a fused multiply-add)
                w = p                                               # what the rule updates: the parameter, or its float32 master
                if self._mastered(group, p):
                    w, g = self.state[p]["master"], g.float()
                if wd != 0.0:
                    g = g + w * wd
                if mom == 0.0:                                      # no state: both rules are p - lr g
                    w.sub_(g * lr)
                elif keras:
                    v, lg = self.state[p][name], g * lr
                    v.mul_(mom).sub_(lg)
                    if nesterov:
                        w.add_(v * mom).sub_(lg)
                    else:
                        w.add_(v)
                else:
                    buf = self.state[p][name]
                    buf.mul_(mom).add_(g)
                    w.sub_((g + buf * mom) * lr if nesterov else buf * lr)
                if w is not p:
                    p.copy_(w)                                      # round to nearest even


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
        return (group["amsgrad"], self._fused, group["master_weights"])

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

    @staticmethod
    def _group_buffers(group):
        return ("m", "v", "vhat") if group["amsgrad"] else ("m", "v")

    def _fusable(self, group):
        return self._fused

    @staticmethod
    def _table(cols, dev, bf16):                             # (no amsgrad: no vhat column)
        return (nat.adam_table_bf16 if bf16 else nat.adam_table)(*cols, *[None] * ((6 if bf16 else 5) - len(cols)), dev)

    @staticmethod
    def _launch(table, blk, gi, group, tick, bf16, clip=None):
        (nat.adam_step_bf16 if bf16 else nat.adam_step)(table, blk, gi, tick=tick, clip=clip)

    def _expressions(self, plans, lr_ts):
        for (_, rest), group, lr_t in zip(plans, self.param_groups, lr_ts):
            b1, b2, eps, wd = float(group["beta_1"]), float(group["beta_2"]), float(group["epsilon"]), float(group["weight_decay"])
            for p in rest:                                          # one rounding per operation, in the kernel's order: no `alpha=`
                st = self.state[p]                                  # forms (the framework evaluates those as a fused multiply-add)
                g = p.grad.to_dense() if p.grad.is_sparse else p.grad
                w = p                                               # what the rule updates: the parameter, or its float32 master
                if self._mastered(group, p):
                    w, g = st["master"], g.float()
                if wd != 0.0:
                    g = g + w * wd
                m, v = st["m"], st["v"]
                m.mul_(b1).add_(g * (1.0 - b1))
                v.mul_(b2).add_((g * g) * (1.0 - b2))
                den = v
                if group["amsgrad"]:
                    den = torch.maximum(st["vhat"], v, out=st["vhat"])
                # (the framework's vectorised CPU sqrt is one ulp off IEEE's on 0.7 % of values; the float64 one rounded to
                #  float32 is the correctly rounded float32 root: 53 >= 2 * 24 + 2 bits, double rounding cannot show)
                root = den.sqrt() if den.dtype == torch.float64 else den.double().sqrt().to(den.dtype)
                w.sub_((m * lr_t) / (root + eps))
                if w is not p:
                    p.copy_(w)                                      # round to nearest even
