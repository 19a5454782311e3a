"""Gradient clipping on the device, bit for bit against tests/np_clip.py: the partials and finish kernels alone, SGD and Adam with
clipnorm / clipvalue over float32 parameters and over bf16 parameters with masters, the cases worked by hand, non-finite gradients
with and without skip_nonfinite, a captured step replayed with changing gradients, the optimizer without the keywords (unchanged, and
no launch added), the refusals, and fit_generator with a clipping optimizer."""
import importlib.util
import itertools
import os

import numpy as np
import pytest

from tests import clip_hand_cases as hand
from tests import np_clip, np_optim, np_sgd
from tests.test_fit_gpu import _batches, _loss, _model
from tests.test_ssd7_fused_training_gpu import _state_equal, deterministic_convolutions  # noqa: F401  (the last one is a fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1, 3, 8, 2047, 2048, 4095, 4097, 8191, 8192, 8193]
CLIP_KEY = "clip_state:cuda:0"


def _nat():
    from ssd_keras_amd import _native as nat
    nat.load()
    return nat


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and bool(np.array_equal(_bits(a), _bits(b)))


def _host(t):
    """A tensor's values in memory order as float32 (bf16 widened exactly)."""
    return t.detach().float().cpu().numpy().reshape(-1)


def _views(torch, arrays, dtype, stagger):
    """The arrays as tensors of `dtype` on the device; with `stagger` views into one buffer that start 0, 1, 2, ... elements past a
    16-byte boundary, so that every load width of the kernel is taken."""
    if not stagger:
        return [torch.from_numpy(a).cuda().to(dtype) for a in arrays]
    per = 16 // torch.empty((), dtype=dtype).element_size()
    out, at, spans = [], 0, []
    for k, a in enumerate(arrays):
        at = -(-at // per) * per + k % per
        spans.append((at, at + a.size))
        at += a.size
    whole = torch.zeros((at + per,), dtype=dtype, device="cuda")
    for (lo, hi), a in zip(spans, arrays):
        whole[lo:hi] = torch.from_numpy(a).cuda().to(dtype)
        out.append(whole[lo:hi])
    return out


# ---- the kernels alone -----------------------------------------------------------------------------------------------------------------
def _kernels_alone(sizes, bf16, weights, weight_decay, stagger, clipnorm):
    import torch
    nat = _nat()
    rng = np.random.RandomState(len(sizes) + 2 * bf16 + weights)
    gs = _views(torch, [rng.randn(n).astype(np.float32) for n in sizes], torch.bfloat16 if bf16 else torch.float32, stagger)
    ws = _views(torch, [rng.randn(n).astype(np.float32) for n in sizes], torch.float32, stagger) if weights else None
    table = nat.grad_sumsq_table(gs, ws, gs[0].device)
    guard = 7
    out = torch.full((table[-1] + 2 * guard,), -1.0, device="cuda")
    nat.grad_sumsq_partials(table, weight_decay, out[guard:guard + table[-1]])
    got = out.cpu().numpy()
    ts = [np_clip.Clip.gradient(_host(g), _host(w) if ws else None, weight_decay if ws else 0.0) for g, w in zip(gs, ws or gs)]
    want = np_clip.partials(ts, 8 if bf16 else 4)
    assert want.size == table[-1] == sum(-(-n // 8192) for n in sizes)
    assert _same_bits(got[guard:-guard], want), np.flatnonzero(_bits(got[guard:-guard]) != _bits(want))
    assert (got[:guard] == -1).all() and (got[-guard:] == -1).all()           # exactly one store per chunk, none outside
    # the finish launch, twice: the counters count, the decision is the last step's
    block = torch.full((nat.clip_state_bytes(),), 0xAB, dtype=torch.uint8, device="cuda")
    nat.clip_state_init(block, clipnorm, 0.0, False)
    ref = np_clip.Clip(clipnorm)
    st = nat.clip_state_read(block)
    assert (st["q"], st["norm"], st["scale"], st["skip"], st["steps"], st["clipped"], st["skipped"]) == (0.0, 0.0, 1.0, 0, 0, 0, 0)
    assert st["clipnorm"] == np.float32(clipnorm) and st["clipvalue"] == 0 and not st["reserved"].any()
    for _ in range(2):
        nat.clip_finish(block, out[guard:guard + table[-1]])
        ref.finish(want)
    st = nat.clip_state_read(block)
    print("q %r norm %r scale %r" % (st["q"], st["norm"], st["scale"]))
    assert _same_bits(st["q"], ref.q) and _same_bits(st["norm"], ref.norm) and _same_bits(st["scale"], ref.scale)
    assert {k: int(st[k]) for k in ("steps", "clipped", "skipped")} == ref.stats and st["skip"] == 0
    return ref


@pytest.mark.parametrize("bf16", [False, True], ids=["float32", "bfloat16"])
@pytest.mark.parametrize("weights", [False, True], ids=["gradient_only", "with_weights"])
@pytest.mark.parametrize("stagger", [False, True], ids=["aligned", "staggered"])
def test_partials_and_finish_over_every_size(bf16, weights, stagger):
    ref = _kernels_alone(SIZES, bf16, weights, 0.375, stagger, clipnorm=150.0)
    assert ref.stats["clipped"] == 2 and ref.scale < 1                        # norm ~ 200 (~ 209 with the weights' share)


def test_a_weight_column_is_not_read_when_weight_decay_is_zero():
    a = _kernels_alone(SIZES[:5], False, True, 0.0, False, clipnorm=1e6)
    b = _kernels_alone(SIZES[:5], False, False, 0.0, False, clipnorm=1e6)
    assert a.stats["clipped"] == b.stats["clipped"] == 0 and a.scale == 1


@pytest.mark.parametrize("bf16", [False, True], ids=["float32", "bfloat16"])
def test_a_table_that_spans_launches(bf16):
    _kernels_alone([5] * 129, bf16, True, 0.5, False, clipnorm=1.0)


def test_kernel_refusals_happen_before_anything_is_launched():
    import torch
    nat = _nat()
    g = [torch.ones(5, device="cuda"), torch.ones(8193, device="cuda")]
    table = nat.grad_sumsq_table(g, None, g[0].device)
    out = torch.full((8,), -1.0, device="cuda")
    for n in (2, 4):                                                          # the table has three chunks
        with pytest.raises(nat.SsdHipError):
            nat.grad_sumsq_partials(table, 0.0, out[:n])
    with pytest.raises(nat.SsdHipError):
        nat.grad_sumsq_partials(table, -1.0, out[:3])
    with pytest.raises(nat.SsdHipError):
        nat.clip_state_init(torch.zeros(80, dtype=torch.uint8, device="cuda")[8:72], 1.0, 0.0, False)   # not 16-byte aligned
    with pytest.raises(nat.SsdHipError):
        nat.clip_state_init(torch.zeros(64, dtype=torch.uint8, device="cuda"), -1.0, 0.0, False)
    torch.cuda.synchronize()
    assert (out == -1).all()


# ---- the optimizers -------------------------------------------------------------------------------------------------------------------
RULES = {
    "sgd_torch": ("sgd", dict(rule="torch")), "sgd_keras": ("sgd", dict(rule="keras")),
    "sgd_torch_nesterov": ("sgd", dict(rule="torch", nesterov=True)), "sgd_keras_nesterov": ("sgd", dict(rule="keras", nesterov=True)),
    "adam": ("adam", {}), "adam_amsgrad": ("adam", dict(amsgrad=True)),
}
GROUP_SIZES = ([5] * 85, [8193, 3, 2048])                                     # 85 tensors: more than any step's tensors per launch
GROUP_WD = (0.0, 0.25)


class _Pair:
    """An optimizer of the package on the device and its NumPy statement, fed the same gradients."""

    def __init__(self, kind, kw, bf16, clip, seed=0, sizes=GROUP_SIZES, wds=GROUP_WD):
        import torch
        from ssd_keras_amd.optimizers import SGD, Adam
        self.torch, self.kind, self.bf16 = torch, kind, bf16
        rng = np.random.RandomState(seed)
        dtype = torch.bfloat16 if bf16 else torch.float32
        self.params = [[torch.nn.Parameter(torch.from_numpy(rng.randn(n).astype(np.float32)).cuda().to(dtype)) for n in ns] for ns in sizes]
        groups = [dict(params=ps, weight_decay=wd) for ps, wd in zip(self.params, wds)]
        if kind == "sgd":
            hyper = dict(lr=0.1, momentum=0.9, decay=0.01, **kw)
            self.opt = SGD(groups, master_weights=bf16, **hyper, **clip)
            self.rules = [np_sgd.SGD(weight_decay=0.0, **hyper) for _ in groups]
            self.names = {"buf": SGD._BUFFER[hyper["rule"]]}
            fresh = np_sgd.fresh
        else:
            hyper = dict(lr=0.01, epsilon=1e-8, decay=0.01, **kw)
            self.opt = Adam(groups, master_weights=bf16, **hyper, **clip)
            self.rules = [np_optim.Adam(weight_decay=0.0, **hyper) for _ in groups]
            self.names = {"m": "m", "v": "v", **({"vhat": "vhat"} if kw.get("amsgrad") else {})}
            fresh = lambda p: np_optim.fresh(p, kw.get("amsgrad", False))
        self.tensors = [[fresh(_host(p)) for p in ps] for ps in self.params]
        self.clip = np_clip.Clip(**clip)
        self.wds = wds

    def set_grads(self, grads, in_place=False):
        """`grads`: per group a list of float32 arrays; a bf16 parameter gets them rounded, and so does the statement."""
        self.grads = []
        for ps, gs in zip(self.params, grads):
            row = []
            for p, g in zip(ps, gs):
                t = self.torch.from_numpy(np.asarray(g, dtype=np.float32)).cuda().to(p.dtype)
                if in_place:
                    p.grad.copy_(t)
                else:
                    p.grad = t
                row.append(_host(t))
            self.grads.append(row)

    def reference_step(self):
        return np_clip.step(self.clip, [dict(rule=r, wd=wd, tensors=ts, grads=gs, vector=8 if self.bf16 else 4)
                                        for r, wd, ts, gs in zip(self.rules, self.wds, self.tensors, self.grads)])

    def check(self, same=_same_bits):
        for ps, ts in zip(self.params, self.tensors):
            for k, (p, t) in enumerate(zip(ps, ts)):
                st = self.opt.state[p]
                assert same(_host(st["master"] if self.bf16 else p), t["p"]), ("p", k)
                if self.bf16:
                    assert self.torch.equal(p.detach().cpu(), self.torch.from_numpy(t["p"]).bfloat16()), ("bf16(master)", k)
                for ours, theirs in self.names.items():
                    assert st[theirs].dtype == self.torch.float32 and same(_host(st[theirs]), t[ours]), (theirs, k)
        assert self.opt.iterations == self.rules[0].iterations == self.rules[-1].iterations
        assert self.opt.clip_stats == self.clip.stats
        norm = self.opt.grad_norm
        assert same(np.float32(norm), self.clip.norm), (norm, self.clip.norm)


def _random_grads(rng, sizes, scale):
    return [[(scale * rng.randn(n)).astype(np.float32) for n in ns] for ns in sizes]


@pytest.mark.parametrize("bf16", [False, True], ids=["float32", "bf16_masters"])
@pytest.mark.parametrize("name", list(RULES))
def test_clipped_optimizer_equals_the_restatement_bit_for_bit(name, bf16):
    """Three steps: the first and third clip (norm ~ 400 against 100), the second does not (~ 25, all of it the penalty's share)."""
    kind, kw = RULES[name]
    clip = dict(clipnorm=100.0, clipvalue=1.5) if "keras" in name or kind == "adam" else dict(clipnorm=100.0)
    pair = _Pair(kind, kw, bf16, clip)
    rng = np.random.RandomState(11)
    norms = []
    for scale in (4.0, 0.01, 4.0):
        pair.set_grads(_random_grads(rng, GROUP_SIZES, scale))
        pair.opt.step()
        pair.reference_step()
        pair.check()
        norms.append(pair.opt.grad_norm)
    print(name, "norms", norms, pair.opt.clip_stats)
    assert pair.opt.clip_stats == {"steps": 3, "clipped": 2, "skipped": 0} and pair.opt.iterations == 3
    assert norms[0] > 100 > norms[1]


@pytest.mark.parametrize("case", hand.CASES, ids=[c["name"] for c in hand.CASES])
def test_hand_cases_on_the_device(case):
    """SGD, rule 'torch', lr 1, momentum 1/2 from a zero buffer: buf = out and p = w - out, both exact."""
    import torch
    from ssd_keras_amd.optimizers import SGD
    nat = _nat()
    p = torch.nn.Parameter(torch.from_numpy(case["w"]).cuda())
    p.grad = torch.from_numpy(case["g"]).cuda()
    opt = SGD([p], lr=1.0, momentum=0.5, weight_decay=case["weight_decay"], clipnorm=case["clipnorm"], clipvalue=case["clipvalue"],
              skip_nonfinite=case["skip_nonfinite"])
    opt.step()
    st = nat.clip_state_read(opt.state[CLIP_KEY])
    assert hand.same(st["q"], case["q"]) and hand.same(st["norm"], case["norm"]) and hand.same(st["scale"], case["scale"])
    assert hand.same(opt.grad_norm, case["norm"])
    assert opt.clip_stats == {"steps": 1, "clipped": int(case["clipped"]), "skipped": int(case["skipped"])}
    buf = _host(opt.state[p]["momentum_buffer"])
    if case["out"] is None:
        assert opt.iterations == 0 and _same_bits(_host(p), case["w"]) and not buf.any()
    else:
        assert opt.iterations == 1 and hand.same(buf, case["out"]) and hand.same(_host(p), case["w"] - case["out"])


@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_non_finite_gradients_as_keras_treats_them(bad):
    """A NaN norm compares false: every gradient goes on as it is, the NaN into its own element only.  An infinite norm gives scale 0:
    the finite gradients become 0, the infinite one NaN."""
    pair = _Pair("sgd", dict(rule="keras"), False, dict(clipnorm=2.0), sizes=([8193, 5], [7]), wds=(0.0, 0.5))
    grads = _random_grads(np.random.RandomState(5), ([8193, 5], [7]), 1.0)
    grads[0][0][8192] = bad                                                   # the second chunk of the first tensor
    before = [t["p"].copy() for ts in pair.tensors for t in ts]
    pair.set_grads(grads)
    pair.opt.step()
    pair.reference_step()
    pair.check(same=hand.same)
    after = [t["p"] for ts in pair.tensors for t in ts]
    assert np.isnan(after[0][8192]) and np.isfinite(after[0][:8192]).all() and np.isfinite(after[1]).all()
    if np.isnan(bad):
        assert pair.opt.clip_stats["clipped"] == 0 and not np.array_equal(after[1], before[1])
    else:                                                                     # scale 0: every finite gradient is 0, nothing else moves
        assert pair.opt.clip_stats["clipped"] == 1 and np.array_equal(after[1], before[1])


@pytest.mark.parametrize("name,bf16", [("sgd_keras_nesterov", False), ("adam_amsgrad", True)])
def test_skip_nonfinite_leaves_everything_as_it_was(name, bf16):
    import torch
    kind, kw = RULES[name]
    sizes = ([4097, 5, 5], [2048])
    clip = dict(clipnorm=50.0, skip_nonfinite=True)
    seen, twin = (_Pair(kind, kw, bf16, clip, sizes=sizes) for _ in range(2))
    rng = np.random.RandomState(3)
    g1, g2 = _random_grads(rng, sizes, 2.0), _random_grads(rng, sizes, 2.0)
    for pair in (seen, twin):
        pair.set_grads(g1)
        pair.opt.step()
    twin.reference_step()
    block = seen.opt.state[[k for k in seen.opt.state if isinstance(k, str) and k.startswith(seen.opt._BLOCK)][0]]
    tensors = [p for ps in seen.params for p in ps] + [t for ps in seen.params for p in ps for t in seen.opt.state[p].values()] + [block]
    before = [t.detach().clone() for t in tensors]
    poisoned = [[g.copy() for g in gs] for gs in g2]
    poisoned[0][1][2] = float("inf")
    seen.set_grads(poisoned)
    seen.opt.step()
    assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(tensors, before))
    assert seen.opt.iterations == 1 and seen.opt.clip_stats == {"steps": 2, "clipped": 1, "skipped": 1}
    assert seen.opt.grad_norm == float("inf")
    for pair in (seen, twin):                                                  # the next finite step: as if the bad one had never been
        pair.set_grads(g2)
        pair.opt.step()
    twin.reference_step()
    twin.check()
    assert seen.opt.iterations == 2
    for ps, qs in zip(seen.params, twin.params):
        for p, q in zip(ps, qs):
            assert torch.equal(p, q) and all(torch.equal(seen.opt.state[p][k], twin.opt.state[q][k]) for k in twin.opt.state[q])


def test_skip_nonfinite_without_clipping_only_decides():
    pair = _Pair("adam", {}, False, dict(skip_nonfinite=True), sizes=([8193, 5], [7]), wds=(0.0, 0.5))
    plain = _Pair("adam", {}, False, {}, sizes=([8193, 5], [7]), wds=(0.0, 0.5))
    grads = _random_grads(np.random.RandomState(8), ([8193, 5], [7]), 1.0)
    for p in (pair, plain):
        p.set_grads(grads)
        p.opt.step()
    pair.reference_step()
    pair.check()
    for ps, qs in zip(pair.params, plain.params):
        assert all(_same_bits(_host(p), _host(q)) for p, q in zip(ps, qs))


def test_a_captured_step_replays_with_the_norm_of_its_own_gradients():
    """Five replays, the gradients rewritten in place between them: each equals the eager optimizer fed the same gradients."""
    import torch
    sizes = ([5] * 70, [8193, 2048])
    clip = dict(clipnorm=100.0, clipvalue=2.0)
    graphed, eager = (_Pair("adam", {}, True, clip, sizes=sizes) for _ in range(2))
    rng = np.random.RandomState(21)
    first = _random_grads(rng, sizes, 1.0)
    graphed.set_grads(first)
    graphed.opt.init_state()
    assert CLIP_KEY in graphed.opt.state
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        graphed.opt.step()
    torch.cuda.synchronize()
    assert graphed.opt.iterations == 0 and graphed.opt.clip_stats["steps"] == 0     # a capture runs nothing
    eager.set_grads(first)
    for scale in (4.0, 0.01, 4.0, 0.02, 3.0):
        grads = _random_grads(rng, sizes, scale)
        graphed.set_grads(grads, in_place=True)
        eager.set_grads(grads, in_place=True)
        graph.replay()
        eager.opt.step()
        graphed.reference_step()
        graphed.check()
        for ps, qs in zip(graphed.params, eager.params):
            for p, q in zip(ps, qs):
                assert torch.equal(p, q) and all(torch.equal(graphed.opt.state[p][k], eager.opt.state[q][k]) for k in eager.opt.state[q])
    assert graphed.opt.clip_stats == eager.opt.clip_stats == {"steps": 5, "clipped": 3, "skipped": 0}


def _graph_nodes(graph):
    spec = importlib.util.spec_from_file_location("time_ssd7_train_step", os.path.join(ROOT, "tools", "time_ssd7_train_step.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool.graph_nodes(graph)


def _captured_kernel_nodes(torch, opt):
    """Kernel nodes of `opt.step()` captured alone; None where the framework or the runtime does not let a graph be read."""
    try:
        graph = torch.cuda.CUDAGraph(keep_graph=True)
    except TypeError:
        return None
    with torch.cuda.graph(graph):
        opt.step()
    torch.cuda.synchronize()
    nodes = _graph_nodes(graph)
    return None if nodes is None else nodes["kernel"]


@pytest.mark.parametrize("name,bf16", [("sgd_torch", False), ("adam", True)])
def test_without_the_keywords_nothing_changes(name, bf16):
    """The optimizer built without the keywords: the unclipped restatement bit for bit over three steps (what it was before the
    keywords existed), and no clip block."""
    kind, kw = RULES[name]
    pair = _Pair(kind, kw, bf16, {})
    for r, wd in zip(pair.rules, GROUP_WD):
        r.weight_decay = wd                                                   # the rule's own term, as ever
    rng = np.random.RandomState(13)
    for scale in (4.0, 0.01, 4.0):
        pair.set_grads(_random_grads(rng, GROUP_SIZES, scale))
        pair.opt.step()
        for r, ts, gs in zip(pair.rules, pair.tensors, pair.grads):
            r.step(ts, gs)
    assert pair.opt.grad_norm is None and pair.opt.clip_stats == {"steps": 0, "clipped": 0, "skipped": 0}
    assert not [k for k in pair.opt.state if isinstance(k, str) and "clip" in k] and not pair.opt._clip_partials
    for ps, ts in zip(pair.params, pair.tensors):
        for p, t in zip(ps, ts):
            assert _same_bits(_host(pair.opt.state[p]["master"] if bf16 else p), t["p"])
    assert pair.opt.iterations == 3


@pytest.mark.parametrize("name,bf16", [("sgd_torch", False), ("adam", True)])
def test_kernel_nodes_of_a_captured_step(name, bf16):
    """Without the keywords a captured `step()` has the kernel nodes it always had.  No count of the parent commit is recorded
    anywhere, so "always had" is the formula of its launches: the tick and one update per 80 (64: Adam on bf16) tensors of a group.
    Clipping adds one partials launch per table and the finish.  Where the framework cannot keep a captured graph readable or the
    runtime does not answer the node query, nothing can be counted and the test says so by skipping."""
    import torch
    kind, kw = RULES[name]
    rng = np.random.RandomState(13)
    counts = {}
    for arm, clip in (("plain", {}), ("clipped", dict(clipnorm=100.0))):
        pair = _Pair(kind, kw, bf16, clip)
        pair.set_grads(_random_grads(rng, GROUP_SIZES, 1.0))
        pair.opt.init_state()
        counts[arm] = _captured_kernel_nodes(torch, pair.opt)
    print("kernel nodes of a captured step: %r" % (counts,))
    if None in counts.values():
        pytest.skip("the nodes of a captured graph are not obtainable here (keep_graph / hipGraphGetNodes): nothing was counted")
    updates = sum(-(-len(ns) // (64 if bf16 else 80)) for ns in GROUP_SIZES)
    assert counts["plain"] == 1 + updates and counts["clipped"] == counts["plain"] + len(GROUP_SIZES) + 1


def test_a_group_that_leaves_the_fused_launch_after_init_state_is_refused():
    """`init_state()` with a momentum, then momentum 0: the parameters would go through the tensor expressions, which do not clip.  The
    refusal is decided at every step, not remembered from `init_state()`."""
    pair = _Pair("sgd", dict(rule="torch"), False, dict(clipnorm=1.0), sizes=([5, 9],), wds=(0.0,))
    pair.set_grads(_random_grads(np.random.RandomState(1), ([5, 9],), 1.0))
    pair.opt.init_state()
    before = [_host(p).copy() for p in pair.params[0]]
    pair.opt.param_groups[0]["momentum"] = 0.0
    with pytest.raises(ValueError, match="parameter 0 of group 0"):
        pair.opt.step()
    assert all(_same_bits(_host(p), b) for p, b in zip(pair.params[0], before)) and pair.opt.clip_stats["steps"] == 0


def test_the_partials_buffer_does_not_move_when_more_parameters_get_gradients():
    """It is sized for every parameter of the optimizer at once: a step captured while only some had gradients keeps a live pointer."""
    sizes = ([8193, 5, 20000],)
    pair = _Pair("adam", {}, False, dict(clipnorm=1.0), sizes=sizes, wds=(0.0,))
    grads = _random_grads(np.random.RandomState(2), sizes, 1.0)
    ps = pair.params[0]
    ps[1].grad = pair.torch.from_numpy(grads[0][1]).cuda()
    pair.opt.init_state()
    (buf,) = pair.opt._clip_partials.values()
    assert buf.numel() == 2 + 1 + 3
    pair.opt.step()
    pair.set_grads(grads)
    pair.opt.step()
    assert list(pair.opt._clip_partials.values())[0] is buf and pair.opt.clip_stats["steps"] == 2


def test_a_bound_that_never_binds_changes_no_bit():
    """clipnorm far above the norm: the multiplication by 1.0f and the clamp that never clamps leave the plain optimizer's result."""
    plain = _Pair("adam", dict(amsgrad=True), True, {})
    bound = _Pair("adam", dict(amsgrad=True), True, dict(clipnorm=1e30, clipvalue=1e30))
    rng = np.random.RandomState(17)
    for _ in range(2):
        grads = _random_grads(rng, GROUP_SIZES, 1.0)
        for pair in (plain, bound):
            pair.set_grads(grads)
            pair.opt.step()
    assert bound.opt.clip_stats == {"steps": 2, "clipped": 0, "skipped": 0}
    for ps, qs in zip(plain.params, bound.params):
        for p, q in zip(ps, qs):
            assert all(_same_bits(_host(plain.opt.state[p][k]), _host(bound.opt.state[q][k])) for k in plain.opt.state[p])


def test_routes_that_do_not_clip_are_refused_before_anything_is_launched():
    import torch
    from ssd_keras_amd.optimizers import SGD, Adam
    f32 = [torch.nn.Parameter(torch.ones(9, device="cuda")) for _ in range(2)]
    b16 = [torch.nn.Parameter(torch.ones(9, device="cuda", dtype=torch.bfloat16)) for _ in range(2)]
    for ps in (f32, b16):
        for p in ps:
            p.grad = torch.ones_like(p)
    cases = [(SGD(f32, lr=0.1, clipnorm=1.0), f32, "parameter 0 of group 0"),                      # momentum 0: tensor expressions
             (SGD(b16, lr=0.1, momentum=0.9, clipvalue=1.0), b16, "parameter 0 of group 0"),       # bf16 without masters
             (Adam(b16, skip_nonfinite=True), b16, "parameter 0 of group 0"),
             (Adam([dict(params=f32), dict(params=b16)], clipnorm=1.0, master_weights=False), b16, "parameter 0 of group 1")]
    for opt, ps, where in cases:
        for call in (opt.step, opt.init_state):
            with pytest.raises(ValueError, match=where):
                call()
        assert not opt.state and not opt._clip_partials
        assert all(bool((p == 1).all()) for p in f32 + b16)


# ---- fit_generator -------------------------------------------------------------------------------------------------------------------
def test_fit_generator_with_a_clipping_optimizer(deterministic_convolutions):  # noqa: F811
    """Two epochs of three steps on the 76 x 68 SSD7, Adam with masters: clipnorm is the median norm of a dry run, so some steps clip
    and some do not; the captured loop equals the eager one bit for bit.  fit_generator itself knows nothing about clipping."""
    import torch
    from ssd_keras_amd.optimizers import Adam
    from ssd_keras_amd.training import fit_generator
    batches = _batches(_model())
    kw = dict(lr=1e-3, epsilon=1e-8, master_weights=True)

    def fit(graph, **clip):
        model = _model()
        opt = Adam(model.parameters(), **kw, **clip)
        hist = fit_generator(model, itertools.cycle(batches), len(batches), 2, optimizer=opt, loss=_loss(), graph=graph)
        return model, opt, hist

    # the dry run: the loop by hand with a bound that never binds, reading the norm of every step
    model, lf = _model(), _loss()
    dry = Adam(model.parameters(), clipnorm=1e30, **kw)
    norms = []
    for img, y in batches * 2:
        dry.zero_grad(set_to_none=True)
        lf.compute_loss(y, model(img).float()).mean().backward()
        dry.step()
        norms.append(dry.grad_norm)
    clipnorm = float(np.median(norms))
    print("norms of the dry run %r, clipnorm %r" % (norms, clipnorm))
    assert all(np.isfinite(norms)) and min(norms) < clipnorm
    g_model, g_opt, g_hist = fit(True, clipnorm=clipnorm)
    e_model, e_opt, e_hist = fit(False, clipnorm=clipnorm)
    print("clip_stats: graph %r, eager %r; norm %r" % (g_opt.clip_stats, e_opt.clip_stats, g_opt.grad_norm))
    assert g_opt.iterations == e_opt.iterations == 6 and g_hist.history == e_hist.history
    assert _state_equal(g_model, e_model)
    for p, q in zip(g_model.parameters(), e_model.parameters()):
        assert all(torch.equal(g_opt.state[p][k], e_opt.state[q][k]) for k in ("master", "m", "v"))
    assert g_opt.clip_stats == e_opt.clip_stats and g_opt.clip_stats["steps"] == 6 and g_opt.clip_stats["clipped"] > 0
    assert g_opt.grad_norm == e_opt.grad_norm
