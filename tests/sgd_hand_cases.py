"""SGD with momentum under both rules of tests/np_sgd.py's docstring: a few steps worked out BY HAND -- what the rules say, not what an
implementation returned.  Every value is a dyadic rational of a few bits, so each float32 (and float64) operation is exact and the
results are compared with ==.  Shared by the CPU tests (the NumPy restatement, the package's tensor-expression path) and the GPU tests
(the kernel).  Each case has two elements, the second with p0 and every gradient multiplied by -2: the rules are linear in (p0, g),
so its expected values are -2 x the first element's (and a sign or lane mix-up shows).

Every case: name, hyperparameters, p0, per step (gradient, learning rate to set before the step or None), and after each step the
expected p and buffer (`buf`: torch's momentum_buffer or Keras's velocity) and, where it is dyadic, lr_t."""

CASES = []


def _case(name, kw, p0, steps):
    """steps: (g, set_lr, p, buf, lr_t) for the first element."""
    two = lambda x: [x, -2.0 * x]
    CASES.append(dict(name=name, kw=kw, p0=two(p0), grads=[two(s[0]) for s in steps], set_lr=[s[1] for s in steps],
                      expect=[dict(p=two(s[2]), buf=two(s[3]), lr_t=s[4]) for s in steps]))


# --- a learning-rate change: lr 1/2, 1/2, 1/4, momentum 1/2, g = 1, p0 = 0.
#   Keras:  v = v/2 - lr g:  v1 = -1/2, p = -1/2;  v2 = -1/4 - 1/2 = -3/4, p = -5/4;  v3 = -3/8 - 1/4 = -5/8, p = -15/8
#   torch:  buf = buf/2 + g: buf1 = 1, p = -1/2;  buf2 = 3/2, p = -1/2 - 3/4 = -5/4;  buf3 = 7/4, p = -5/4 - 7/16 = -27/16
#   (equal while the rate is constant; the velocity keeps the old rate on its history, the buffer is rescaled as a whole)
_case("rate_change_keras", dict(lr=0.5, momentum=0.5, rule="keras"), 0.0,
      [(1.0, None, -0.5, -0.5, 0.5), (1.0, None, -1.25, -0.75, 0.5), (1.0, 0.25, -1.875, -0.625, 0.25)])
_case("rate_change_torch", dict(lr=0.5, momentum=0.5, rule="torch"), 0.0,
      [(1.0, None, -0.5, 1.0, 0.5), (1.0, None, -1.25, 1.5, 0.5), (1.0, 0.25, -1.6875, 1.75, 0.25)])

# --- Nesterov, lr 1/2, momentum 1/2, g = 1, p0 = 0.
#   torch:  buf1 = 1, d = 1 + 1/2 = 3/2, p = -3/4;  buf2 = 3/2, d = 1 + 3/4 = 7/4, p = -3/4 - 7/8 = -13/8
#   Keras:  v1 = -1/2, p = (0 - 1/4) - 1/2 = -3/4;  v2 = -1/4 - 1/2 = -3/4, p = (-3/4 - 3/8) - 1/2 = -13/8
_case("nesterov_torch", dict(lr=0.5, momentum=0.5, nesterov=True, rule="torch"), 0.0,
      [(1.0, None, -0.75, 1.0, 0.5), (1.0, None, -1.625, 1.5, 0.5)])
_case("nesterov_keras", dict(lr=0.5, momentum=0.5, nesterov=True, rule="keras"), 0.0,
      [(1.0, None, -0.75, -0.5, 0.5), (1.0, None, -1.625, -0.75, 0.5)])

# --- decay = 1, lr0 = 1/2: the step at count t runs at lr0 / (1 + (t - 1)) = 1/2, 1/4, 1/6, 1/8.  The third rate is no dyadic number, so
#   the third step is arranged not to see it; momentum 1/2.
#   Keras, g = (1, 1, 0, 1): v1 = -1/2, p = -1/2;  v2 = -1/4 - 1/4 = -1/2, p = -1;  v3 = -1/4 - lr 0 = -1/4, p = -5/4;
#                            v4 = -1/8 - 1/8 = -1/4, p = -3/2
#   torch, g = (1, 1, -3/4, 1): buf1 = 1, p = -1/2;  buf2 = 3/2, p = -1/2 - 3/8 = -7/8;  buf3 = 3/4 - 3/4 = 0, p = -7/8 - lr 0;
#                            buf4 = 1, p = -7/8 - 1/8 = -1
_case("decay_keras", dict(lr=0.5, momentum=0.5, decay=1.0, rule="keras"), 0.0,
      [(1.0, None, -0.5, -0.5, 0.5), (1.0, None, -1.0, -0.5, 0.25), (0.0, None, -1.25, -0.25, None), (1.0, None, -1.5, -0.25, 0.125)])
_case("decay_torch", dict(lr=0.5, momentum=0.5, decay=1.0, rule="torch"), 0.0,
      [(1.0, None, -0.5, 1.0, 0.5), (1.0, None, -0.875, 1.5, 0.25), (-0.75, None, -0.875, 0.0, None), (1.0, None, -1.0, 1.0, 0.125)])

# --- weight_decay = 1/2, lr 1/2, momentum 1/2, p0 = 2, g = 1: g' = g + p/2.
#   step 1: g' = 2.  torch: buf = 2, p = 2 - 1 = 1.        Keras: v = -1, p = 1
#   step 2: g' = 1 + 1/2 = 3/2.  torch: buf = 1 + 3/2 = 5/2, p = 1 - 5/4 = -1/4.   Keras: v = -1/2 - 3/4 = -5/4, p = -1/4
_case("weight_decay_torch", dict(lr=0.5, momentum=0.5, weight_decay=0.5, rule="torch"), 2.0,
      [(1.0, None, 1.0, 2.0, 0.5), (1.0, None, -0.25, 2.5, 0.5)])
_case("weight_decay_keras", dict(lr=0.5, momentum=0.5, weight_decay=0.5, rule="keras"), 2.0,
      [(1.0, None, 1.0, -1.0, 0.5), (1.0, None, -0.25, -1.25, 0.5)])

BUFFER = {"torch": "momentum_buffer", "keras": "velocity"}     # the package's state key of `buf`
