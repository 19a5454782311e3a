"""keras.optimizers.Optimizer.get_gradients / clip_norm of Keras 2.2.4, RESTATED in NumPy -- neither Keras nor TensorFlow exists where
this project runs, so this is what their source says, as tests/np_sgd.py and tests/np_optim.py are for the update rules:

    grads = K.gradients(loss, params)
    if self.clipnorm > 0:
        norm = K.sqrt(sum([K.sum(K.square(g)) for g in grads]))                ONE norm over all parameters
        grads = [clip_norm(g, self.clipnorm, norm) for g in grads]             g * clipnorm / norm  if norm >= clipnorm  else g
    if self.clipvalue > 0:
        grads = [K.clip(g, -self.clipvalue, self.clipvalue) for g in grads]    minimum / maximum: a NaN stays a NaN

with the conventions of include/ssdhip.h written out.  `loss` is the PENALISED loss, so g is t = g + weight_decay * w (two float32
operations; w the float32 parameter or master).  The norm: float32 partials of t * t per chunk of 8192 elements in the order of
additions of ssdhip_sumsq_partials (tests/np_fit.py), q = their float64 sum in index order, norm = float32(sqrt(q)),
scale = clipnorm / norm as ONE float32 division when norm >= clipnorm, else 1.0 -- and the multiplication by scale always happens when
clipnorm is on.  A NaN norm compares false and clips nothing; an infinite norm gives scale 0.  `skip_nonfinite` is the project's own:
a step whose q is not finite does nothing at all and is counted."""
import numpy as np

from tests import np_fit


class Clip:
    """struct ssdhip_clip_state after ssdhip_clip_state_init, ssdhip_clip_finish as `finish`, the clipped update's first three
    operations as `gradient` and `apply`."""

    def __init__(self, clipnorm=None, clipvalue=None, skip_nonfinite=False):
        self.clipnorm, self.clipvalue = np.float32(clipnorm or 0.0), np.float32(clipvalue or 0.0)
        self.skip_nonfinite = bool(skip_nonfinite)
        self.q, self.norm, self.scale, self.skip = np.float64(0.0), np.float32(0.0), np.float32(1.0), False
        self.steps = self.clipped = self.skipped = 0

    @staticmethod
    def gradient(g, w, weight_decay):
        """t = g + weight_decay * w in float32 (g float32, or bf16 values widened); t = g when weight_decay == 0."""
        t = np.asarray(g, dtype=np.float32)
        if weight_decay != 0.0:
            with np.errstate(all="ignore"):
                t = (t + (np.float32(weight_decay) * np.asarray(w, dtype=np.float32)).astype(np.float32)).astype(np.float32)
        return t

    def finish(self, partials):
        q = np.float64(0.0)
        for v in np.asarray(partials, dtype=np.float32):   # index order, float64
            q = q + np.float64(v)
        with np.errstate(all="ignore"):
            norm = np.float32(np.sqrt(q))
            clip = bool(self.clipnorm > 0 and norm >= self.clipnorm)
            scale = np.float32(self.clipnorm / norm) if clip else np.float32(1.0)
        self.q, self.norm, self.scale = q, norm, scale
        self.skip = self.skip_nonfinite and not np.isfinite(q)
        self.steps += 1
        if self.skip:
            self.skipped += 1
        elif clip:
            self.clipped += 1

    def apply(self, t):
        with np.errstate(all="ignore"):
            if self.clipnorm > 0:
                t = (t * self.scale).astype(np.float32)
            if self.clipvalue > 0:
                t = np.where(t > self.clipvalue, self.clipvalue, t)      # comparisons: a NaN goes through both
                t = np.where(t < -self.clipvalue, -self.clipvalue, t)
        return t.astype(np.float32)

    @property
    def stats(self):
        return {"steps": self.steps, "clipped": self.clipped, "skipped": self.skipped}


def partials(ts, vector):
    """The float32 partials of one tensor table: `ts` its completed gradients, `vector` 4 (float32 gradients) or 8 (bf16)."""
    return np_fit.sumsq_kernel_order(ts, vector)


def step(clip, groups):
    """One clipped optimizer step.  `groups`: dicts {"rule": an np_sgd.SGD / np_optim.Adam built with weight_decay 0 (the term is
    applied here, once), "wd": the group's weight decay, "tensors": its list of state dicts ("p" the float32 parameter or master),
    "grads": the gradients (float32 arrays; bf16 gradients as their float32 values), "vector": 4 or 8}.  One table per group, in order.
    Returns the completed, clipped gradients per group (None on a skipped step)."""
    ts = [[clip.gradient(g, s["p"], G["wd"]) for s, g in zip(G["tensors"], G["grads"])] for G in groups]
    clip.finish(np.concatenate([partials(t, G["vector"]) for t, G in zip(ts, groups)]))
    if clip.skip:
        return None
    out = [[clip.apply(x) for x in t] for t in ts]
    with np.errstate(all="ignore"):
        for G, t in zip(groups, out):
            assert G["rule"].weight_decay == 0.0
            G["rule"].step(G["tensors"], t)
    return out
