"""Inputs for the SSD loss kernels built straight from NumPy, no encoder: tests/test_loss_cases_cpu.py checks the table against
the oracle and `ssdhip_loss_plan` alone, tests/test_loss_paths_gpu.py runs it on the device.

`from_levels` writes the background prediction q[b, n] of every anchor.  A background anchor's loss is -log(q): anchors with the
SAME q tie exactly on any device (the same float32 goes through the same logf), and levels whose losses lie at least MIN_STEPS
float32 steps apart cannot change order under a logf that is a few ulp from NumPy's log.  So the hard-negative mask of such a
case is the oracle's, bit for bit: no knife-edge flips to allow for.

A Case names its shape, the loss options, and what it is for; `build()` makes (y_true, y_pred), `oracle()` the reference
results.  Both are computed once per process and must be left unchanged by whoever uses them."""
import functools

import numpy as np

MIN_STEPS = 64                # distinct non-zero negative losses are at least this many float32 steps apart
CHUNK = 2048                  # values per select pass block (SELP_CHUNK in csrc/ssdhip_loss.hip)
ITEMS = 8                     # consecutive values per thread of the tie search

# well separated background predictions for the cases that are about the per-anchor kernels, not the select
PATH_LEVELS = np.array([0.05, 0.1, 0.2, 0.3, 0.45, 0.6, 0.75, 0.9], dtype=np.float32)


def from_levels(B, N, C, q, positives=None, neutral=None, seed=0):
    """(y_true, y_pred), float32 (B, N, C + 12).  q (B, N): y_pred[..., 0].  positives (B, N) bool: one-hot in a class >= 1,
    everything else is background (t[0] = 1) unless `neutral` (all-zero class vector: the anchor counts nowhere).  The rest of
    the probability, 1 - q, is spread unevenly over the other classes; offsets are N(0, 0.5) on both sides (|difference| on both
    sides of 1, the two branches of smooth L1); the last 8 columns hold arbitrary non-zero numbers, different in y_true and y_pred:
    nothing may read them."""
    rng = np.random.RandomState(seed)
    q = np.broadcast_to(np.asarray(q, dtype=np.float32), (B, N))
    pos = np.zeros((B, N), bool) if positives is None else np.asarray(positives, bool)
    neu = np.zeros((B, N), bool) if neutral is None else np.asarray(neutral, bool) & ~pos
    L = C + 12
    y_true = np.zeros((B, N, L), dtype=np.float32)
    y_pred = np.zeros((B, N, L), dtype=np.float32)
    cls = rng.randint(1, C, size=(B, N))
    cls[~pos] = 0
    y_true[..., :C] = np.eye(C, dtype=np.float32)[cls]
    y_true[neu, :C] = 0
    w = rng.uniform(0.5, 1.5, size=(B, N, C - 1)).astype(np.float32)
    w /= w.sum(axis=-1, keepdims=True)
    y_pred[..., 0] = q
    y_pred[..., 1:C] = w * (np.float32(1) - q)[..., None]
    y_true[..., C:C + 4] = rng.normal(0, 0.5, size=(B, N, 4))
    y_pred[..., C:C + 4] = rng.normal(0, 0.5, size=(B, N, 4))
    for y in (y_true, y_pred):
        y[..., C + 4:] = rng.uniform(1, 3, size=(B, N, 8)) * rng.choice([-1.0, 1.0], size=(B, N, 8))
    return y_true, y_pred


def softmax_inputs(B, N, C, seed):
    """Random softmax predictions (the style of tests/test_loss_gpu.py): the losses are all different, elements ON the cut may flip."""
    rng = np.random.RandomState(seed)
    pos = rng.uniform(size=(B, N)) < 0.05
    y_true, y_pred = from_levels(B, N, C, 0.5, pos, seed=seed)
    z = rng.normal(0, 2, size=(B, N, C))
    e = np.exp(z - z.max(axis=-1, keepdims=True))
    y_pred[..., :C] = (e / e.sum(axis=-1, keepdims=True)).astype(np.float32)
    return y_true, y_pred


class Case:
    def __init__(self, name, shape, make, purpose, exact=True, **kw):
        self.name, self.shape, self._make, self.purpose, self.exact = name, tuple(shape), make, purpose, exact
        self.kw = dict(dict(neg_pos_ratio=3, n_neg_min=0, alpha=1.0), **kw)

    def __repr__(self):
        return self.name

    @functools.lru_cache(maxsize=None)
    def build(self):
        y_true, y_pred = self._make(*self.shape)
        assert y_true.shape == y_pred.shape == self.shape[:2] + (self.shape[2] + 12,)
        for y in (y_true, y_pred):
            y.setflags(write=False)
        return y_true, y_pred

    @functools.lru_cache(maxsize=None)
    def oracle(self):
        """(loss (B,), parts dict of oracle.np_oracle.ssd_loss)."""
        from oracle import np_oracle as orc
        y_true, y_pred = self.build()
        return orc.ssd_loss(y_true, y_pred, return_parts=True, **self.kw)

    def oracle_grad(self):
        """Not kept: 30 MB for the large shapes, and one test per case asks for it."""
        from oracle import np_oracle as orc
        y_true, y_pred = self.build()
        return orc.ssd_loss_grad(y_true, y_pred, grad_out(self.shape[0]), **self.kw)


def grad_out(B):
    """The non-uniform d objective / d loss[b] every gradient test uses."""
    return np.linspace(0.5, 1.5, B).astype(np.float32)


# --------------------------------------------------------------------------------------------------------------------------------
# path cases: every form of the per-anchor kernels
# --------------------------------------------------------------------------------------------------------------------------------
def _path(seed, p_pos=0.1, p_neutral=0.05):
    def make(B, N, C):
        rng = np.random.RandomState(1000 + seed)
        q = PATH_LEVELS[rng.randint(0, len(PATH_LEVELS), size=(B, N))]
        pos = rng.uniform(size=(B, N)) < p_pos
        pos[0, 0] = pos[B - 1, N - 1] = True               # a positive in the first and in the last anchor: n_pos > 0 everywhere
        neu = rng.uniform(size=(B, N)) < p_neutral
        return from_levels(B, N, C, q, pos, neu, seed=seed)
    return make


PATH = [
    Case("smallest", (1, 4, 2), _path(1), "smallest possible: one streaming tile of 4 anchors, three idle waves"),
    Case("one_tile", (1, 64, 2), _path(2), "one full streaming tile, three idle waves; C == 2 (the backward's class maximum starts at 2)"),
    Case("n37", (2, 37, 2), _path(3), "N < 64 and N % 4 != 0: tiled; image 1 starts at 16-byte phase 2"),
    Case("phases", (3, 341, 5), _path(4), "L = 17, N odd: phases 0..3 over images and tiles, TA = 256 with a second tile of 85"),
    Case("tail4", (2, 68, 4), _path(5), "last streaming tile of 4 anchors; C % 4 == 0: no class remainder loop"),
    Case("c7", (2, 60, 7), _path(6), "C % 4 == 3"),
    Case("many_images", (70, 12, 3), _path(7), "many images with one short tile each", n_neg_min=5),
    Case("l36", (2, 132, 24), _path(8), "L = 36: the last streaming row length, 144 KiB of LDS by opt-in"),
    Case("l37", (2, 132, 25), _path(9), "L = 37: the first row length that falls back, TA = 128"),
    Case("ssd300_rows", (2, 130, 21), _path(10), "the ssd300 row length with N L % 4 != 0: tiled, TA = 128", neg_pos_ratio=2, alpha=0.5),
]
WIDE = [
    Case("wide116", (2, 70, 116), _path(11), "L = 128: the first tiled launch above 64 KiB of dynamic LDS, TA = 64"),
    Case("wide250", (1, 70, 250), _path(12), "L = 262: 131 KiB of dynamic LDS"),
]
STREAM33 = Case("l33", (2, 132, 21), _path(13), "the ssd300 row length, streaming")
SOFTMAX = [
    Case("softmax_phases", (3, 341, 5), lambda B, N, C: softmax_inputs(B, N, C, 21), "random softmax rows on the phase shape", exact=False),
    Case("softmax_l36", (2, 132, 24), lambda B, N, C: softmax_inputs(B, N, C, 22), "random softmax rows, streaming", exact=False),
]

# --------------------------------------------------------------------------------------------------------------------------------
# select cases (C = 2)
# --------------------------------------------------------------------------------------------------------------------------------
BIG = (3, 180001, 2)
BIG_TOTAL = BIG[0] * BIG[1]
BIG_KS = (1, 7, 8, 9, 2047, 2048, 2049, 524287, 524288, 524289, BIG_TOTAL - 1, BIG_TOTAL)


@functools.lru_cache(maxsize=None)
def _all_ties_inputs():
    y_true, y_pred = from_levels(*BIG, 0.5, seed=31)
    for y in (y_true, y_pred):
        y.setflags(write=False)
    return y_true, y_pred


def _all_ties(K):
    """Every anchor a background with one q: the mask is exactly the flat indices < K."""
    return Case("all_ties_%d" % K, BIG, lambda B, N, C: _all_ties_inputs(), "K = %d of %d ties" % (K, BIG_TOTAL),
                neg_pos_ratio=0, n_neg_min=K)


ALL_TIES = [_all_ties(K) for K in BIG_KS]

INTERLEAVED_WANT = 520000     # ties to keep besides every higher loss: the 520000th of a 98 % dense tie list lies past 256 * 2048


def _interleaved(B, N, C):
    rng = np.random.RandomState(32)
    high = rng.uniform(size=(B, N)) < 0.02
    return from_levels(B, N, C, np.where(high, np.float32(0.05), np.float32(0.5)), seed=32)


def _interleaved_k():
    rng = np.random.RandomState(32)
    return int((rng.uniform(size=BIG[:2]) < 0.02).sum()) + INTERLEAVED_WANT


INTERLEAVED = Case("interleaved_ties", BIG, _interleaved, "2 % higher losses scattered among the ties: tie rank != flat index, cut in a pass block >= 256",
                   neg_pos_ratio=0, n_neg_min=_interleaved_k())

LEVEL_SHAPE = (2, 6148, 2)
LEVEL3_Q = (np.float64(0.3002) * (1 - 2e-5 * np.arange(12))).astype(np.float32)


def _scatter(B, N, seed, q_levels, p_high=0.02, p_pos=0.05):
    rng = np.random.RandomState(seed)
    q = np.asarray(q_levels, np.float32)[rng.randint(0, len(q_levels), size=(B, N))]
    q[rng.uniform(size=(B, N)) < p_high] = np.float32(0.01)
    pos = rng.uniform(size=(B, N)) < p_pos
    return q, pos


def _level3(B, N, C):
    q, pos = _scatter(B, N, 33, LEVEL3_Q)
    return from_levels(B, N, C, q, pos, seed=33)


LEVEL3 = Case("level3", LEVEL_SHAPE, _level3, "12 losses in one 20-bit key prefix, the cut on one of them with ties on both sides")

LEVEL2_LOSSES = 0.5 + 1.5 * (np.arange(40) + 0.5) / 40       # in [0.5, 2): one top key byte (0x3F | sign), the middle 12 bits all over
LEVEL2_Q = np.exp(-LEVEL2_LOSSES).astype(np.float32)


def _level2(B, N, C):
    q, pos = _scatter(B, N, 34, LEVEL2_Q)
    return from_levels(B, N, C, q, pos, seed=34)


LEVEL2 = Case("level2", LEVEL_SHAPE, _level2, "40 losses sharing the top 8 key bits, spread over the middle 12, with ties on the cut", neg_pos_ratio=10)

UNNORM_SHAPE = (3, 4099, 2)


def _unnormalised(B, N, C):
    """A third of the backgrounds at q = 1.0 (loss 0), a third at 1.5 (loss < 0), a third at 0.25; positives (q = 0.25) every 7th
    anchor and in the last five of every image.  With ratio 1000, k = the number of non-zero negative losses: every positive loss is
    kept, then zeros in flat order, and no negative loss."""
    n = np.arange(B * N).reshape(B, N)
    pos = (n % 7 == 3) | (np.arange(N)[None, :] >= N - 5)
    q = np.choose(n % 3, [np.float32(1.0), np.float32(1.5), np.float32(0.25)]).astype(np.float32)
    q[pos] = np.float32(0.25)
    return from_levels(B, N, C, q, pos, seed=35)


UNNORMALISED = Case("unnormalised", UNNORM_SHAPE, _unnormalised, "the cut falls among zero losses of both signs", neg_pos_ratio=1000)

SELECT = ALL_TIES + [INTERLEAVED, LEVEL3, LEVEL2, UNNORMALISED]
LEVEL_CASES = PATH + WIDE + [STREAM33, INTERLEAVED, LEVEL3, LEVEL2, UNNORMALISED, ALL_TIES[0]]     # where "no knife edges" must hold
ALL = PATH + WIDE + [STREAM33] + SOFTMAX + SELECT

# the payloads that are also run from views 4, 8 and 12 bytes into a larger buffer: (case, y_true offset, y_pred offset)
MISALIGNED = [(c, ot, op) for c in (PATH[4], PATH[7]) for ot, op in ((4, 4), (8, 0), (0, 12), (12, 8))]


# --------------------------------------------------------------------------------------------------------------------------------
# what the oracle says about a case
# --------------------------------------------------------------------------------------------------------------------------------
def float_key(x):
    """The order-preserving key of csrc/ssdhip_math.h for float32 values."""
    u = np.asarray(x, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def min_step_gap(neg_all):
    """The smallest distance, in float32 steps, between two distinct non-zero values of neg_all (inf with fewer than two)."""
    v = np.unique(np.asarray(neg_all, np.float32).reshape(-1))
    v = v[v != 0]
    if v.size < 2:
        return np.inf
    k = np.sort(float_key(v).astype(np.int64))
    return int(np.diff(k).min())


def cut(case):
    """Where the oracle's selection ends: dict with thr (the k-th largest negative loss), ties (how many values equal it), kept (how
    many of those are kept), last (flat index of the last kept tie), block (its pass block) and lane_item (its place in a thread's 8)."""
    _, parts = case.oracle()
    neg = parts["neg_all"].reshape(-1)
    keep = parts["keep"].reshape(-1).astype(bool)
    assert parts["k"] > 0 and keep.sum() == parts["k"]
    thr = neg[keep].min()
    tie = neg == thr
    assert not (keep & (neg < thr)).any() and keep[neg > thr].all()
    last = int(np.flatnonzero(tie & keep)[-1])
    return dict(thr=thr, ties=int(tie.sum()), kept=int((tie & keep).sum()), last=last, block=last // CHUNK, lane_item=last % ITEMS)


def plan(lib, case=None, shape=None, y_true=0, y_pred=0, grad=0, keep=0):
    """ssdhip_loss_plan for a case's shape and operand offsets from a 16-byte boundary -> dict."""
    import ctypes
    B, N, C = shape or case.shape
    out = (ctypes.c_int * 8)()
    base = 1 << 20
    rc = lib.ssdhip_loss_plan(base + y_true, base + y_pred, base + grad, base + keep, B, N, C, out)
    assert rc == 0, rc
    return dict(zip(("fwd_stream", "bwd_stream", "TA", "G", "grid", "waves", "nblk", "gx"), list(out)))
