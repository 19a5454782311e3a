"""keras.optimizers.SGD.get_updates of Keras 2.x (the reference's Keras generation) and torch.optim.SGD's rule, RESTATED in NumPy --
neither Keras nor TensorFlow exists where this project runs, so this is what their source says, as tests/np_optim.py is for Adam:

    lr = self.lr * (1. / (1. + self.decay * iterations))                       (only when decay > 0; `iterations` BEFORE its increment)
    v = self.momentum * m - lr * g                                             (m: the velocity)
    new_p = p + self.momentum * v - lr * g   if self.nesterov   else   p + v

and torch.optim.SGD (dampening 0):

    buf = momentum * buf + g                                                   (the first step's buf = g: the buffer starts as zeros)
    g = g + momentum * buf   if nesterov   else   buf
    p = p - lr * g

with the conventions of csrc/ssdhip_optim.hip (sgd_tick_kernel, sgd_step_kernel) written out: the tick runs in float64,
`lr = lr0 / (1 + decay * (t - 1))` at step t, and lr_t is that value rounded once to the dtype of the arrays; the element arithmetic runs
in the dtype of the arrays, every scalar rounded once to that dtype, one operation at a time in the order above (Keras's Nesterov form
as `(p + momentum * v) - lr * g`, the product `lr * g` taken once).  `weight_decay` adds `weight_decay * p` to the gradient first
(Keras's l2 kernel regulariser as the optimizer sees it).  Both rules are given the time-based decay and both Nesterov forms."""
import numpy as np


class SGD:
    def __init__(self, lr=0.01, momentum=0.0, weight_decay=0.0, decay=0.0, nesterov=False, rule="torch", iterations=0):
        assert rule in ("torch", "keras")
        self.lr, self.momentum, self.weight_decay, self.decay = float(lr), float(momentum), float(weight_decay), float(decay)
        self.nesterov, self.rule = bool(nesterov), rule
        self.iterations, self.lr_t = int(iterations), None

    def tick(self):
        """The scalars of the next step (sgd_tick_kernel): float64, one operation at a time."""
        self.iterations += 1
        lr = self.lr
        if self.decay > 0.0:
            lr = lr / (1.0 + self.decay * float(self.iterations - 1))
        self.lr_t = lr
        return lr

    def update(self, p, g, buf):
        """One tensor's update with the scalars of the last tick; returns the new (p, buf) in p's dtype."""
        dt = p.dtype.type
        lr, mom, wd = dt(self.lr_t), dt(self.momentum), dt(self.weight_decay)
        g = g.astype(p.dtype)
        if self.weight_decay != 0.0:
            g = g + wd * p
        if self.rule == "torch":
            buf = mom * buf + g
            if self.nesterov:
                d = g + mom * buf
                p = p - lr * d
            else:
                p = p - lr * buf
        else:
            lg = lr * g
            buf = mom * buf - lg
            if self.nesterov:
                p = (p + mom * buf) - lg
            else:
                p = p + buf
        assert p.dtype == buf.dtype == g.dtype
        return p, buf

    def step(self, tensors, grads):
        """`tensors`: a list of dicts {"p", "buf"} of arrays (buf zeros before the first step), updated in place."""
        self.tick()
        for t, g in zip(tensors, grads):
            t["p"], t["buf"] = self.update(t["p"], g, t["buf"])


def fresh(p):
    """The state of a parameter before its first step."""
    p = np.array(p)
    return {"p": p, "buf": np.zeros_like(p)}
