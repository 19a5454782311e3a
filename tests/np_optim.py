"""keras.optimizers.Adam.get_updates of Keras 2.x (the reference's Keras generation), RESTATED in NumPy -- neither Keras nor TensorFlow
exists where this project runs, so this is what their source says, as oracle/np_oracle.py's loss is:

    lr = self.lr * (1. / (1. + self.decay * iterations))                       (only when decay > 0; `iterations` BEFORE its increment)
    t = iterations + 1
    lr_t = lr * (K.sqrt(1. - K.pow(self.beta_2, t)) / (1. - K.pow(self.beta_1, t)))
    m_t = (self.beta_1 * m) + (1. - self.beta_1) * g
    v_t = (self.beta_2 * v) + (1. - self.beta_2) * K.square(g)
    vhat_t = K.maximum(vhat, v_t)                                             (amsgrad; vhat_t then stands for v_t below)
    p_t = p - lr_t * m_t / (K.sqrt(v_t) + self.epsilon)

with the two conventions of csrc/ssdhip_adam.hip written out: the scalars are float64, the powers RUNNING PRODUCTS (b^t = b^(t-1) * b, one
multiplication per step: reproducible to the bit, which pow() is not) and `lr = lr0 / (1 + decay * (t - 1))`; the element arithmetic
runs in the dtype of the arrays, every scalar rounded once to that dtype, one operation at a time in the order above.  `weight_decay`
adds `weight_decay * p` to the gradient first (Keras's l2 kernel regulariser as the optimizer sees it)."""
import math

import numpy as np


class Adam:
    def __init__(self, lr=0.001, beta_1=0.9, beta_2=0.999, epsilon=None, decay=0.0, amsgrad=False, weight_decay=0.0, iterations=0):
        self.lr, self.beta_1, self.beta_2 = float(lr), float(beta_1), float(beta_2)
        self.epsilon = 1e-7 if epsilon is None else float(epsilon)
        self.decay, self.amsgrad, self.weight_decay = float(decay), bool(amsgrad), float(weight_decay)
        self.iterations, self.b1t, self.b2t, self.lr_t = 0, 1.0, 1.0, None
        for _ in range(iterations):                        # a restored optimizer: the same sequence of products
            self.iterations += 1
            self.b1t = self.b1t * self.beta_1
            self.b2t = self.b2t * self.beta_2

    def tick(self):
        """The scalars of the next step (adam_tick_kernel): float64, one operation at a time."""
        self.iterations += 1
        self.b1t = self.b1t * self.beta_1
        self.b2t = self.b2t * self.beta_2
        lr = self.lr
        if self.decay > 0.0:
            lr = lr / (1.0 + self.decay * float(self.iterations - 1))
        self.lr_t = lr * math.sqrt(1.0 - self.b2t) / (1.0 - self.b1t)
        return self.lr_t

    def update(self, p, g, m, v, vhat=None):
        """One tensor's update with the scalars of the last tick; returns the new (p, m, v, vhat) in p's dtype."""
        dt = p.dtype.type
        lr_t, b1, b2, eps, wd = dt(self.lr_t), dt(self.beta_1), dt(self.beta_2), dt(self.epsilon), dt(self.weight_decay)
        omb1, omb2 = dt(1.0 - self.beta_1), dt(1.0 - self.beta_2)
        g = g.astype(p.dtype)
        if self.weight_decay != 0.0:
            g = g + wd * p
        m = b1 * m + omb1 * g
        v = b2 * v + omb2 * (g * g)
        den = v
        if self.amsgrad:
            vhat = np.maximum(vhat, v)
            den = vhat
        p = p - lr_t * m / (np.sqrt(den) + eps)
        assert p.dtype == m.dtype == v.dtype == g.dtype
        return p, m, v, vhat

    def step(self, tensors, grads):
        """`tensors`: a list of dicts {"p", "m", "v", "vhat"} of arrays (m, v, vhat zeros before the first step), updated in place."""
        self.tick()
        for t, g in zip(tensors, grads):
            t["p"], t["m"], t["v"], t["vhat"] = self.update(t["p"], g, t["m"], t["v"], t.get("vhat"))


def fresh(p, amsgrad=False):
    """The state of a parameter before its first step."""
    p = np.array(p)
    return {"p": p, "m": np.zeros_like(p), "v": np.zeros_like(p), "vhat": np.zeros_like(p) if amsgrad else None}
