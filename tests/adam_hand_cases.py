"""Keras 2.x Adam: two steps on a handful of values worked out BY HAND in exact fractions from the update rule in tests/np_optim.py's
docstring -- what the rule says, not what an implementation returned.  Shared by the CPU tests (the NumPy restatement, the package's
tensor-expression path) and the GPU tests (the kernel).  Hyperparameters are chosen so that every quantity is a rational number:
beta_2 = 0 makes sqrt(1 - b2^t) = 1, and with beta_2 = 3/4 the gradients are chosen so that the sqrt(7) of step 2 cancels.

Every case: name, hyperparameters, p0, the gradients of each step, and after each step the expected p, m, v (and vhat)."""
from fractions import Fraction as F

CASES = []

# --- beta_1 = 1/2, beta_2 = 3/4, epsilon = 0, lr = 1/4.
#   step 1: b1^1 = 1/2, b2^1 = 3/4: lr_t = lr sqrt(1/4) / (1/2) = lr.  m = g/2, v = g^2/4, sqrt(v) = |g|/2: p -= lr sign(g).
#     g = (2, 4, -1): m = (1, 2, -1/2), v = (1, 4, 1/4), p = (1 - 1/4, -2 - 1/4, 1/2 + 1/4) = (3/4, -9/4, 3/4)
#   step 2: b1^2 = 1/4, b2^2 = 9/16: lr_t = lr sqrt(7/16) / (3/4) = lr sqrt(7) / 3.  g = (2, -4, -1) (|g| as in step 1):
#     m = m/2 + g/2 = (3/2, -1, -3/4);  v = 3/4 v + g^2/4 = (7/4, 7, 7/16), sqrt(v) = sqrt(7) (1/2, 1, 1/4)
#     m / sqrt(v) = (3, -1, -3) / sqrt(7);  update = lr/3 (3, -1, -3) = (1/4, -1/12, -1/4);  p = (1/2, -13/6, 1)
CASES.append(dict(
    name="sqrt7_cancels", kw=dict(lr=F(1, 4), beta_1=F(1, 2), beta_2=F(3, 4), epsilon=0),
    p0=[F(1), F(-2), F(1, 2)], grads=[[F(2), F(4), F(-1)], [F(2), F(-4), F(-1)]],
    expect=[dict(p=[F(3, 4), F(-9, 4), F(3, 4)], m=[F(1), F(2), F(-1, 2)], v=[F(1), F(4), F(1, 4)]),
            dict(p=[F(1, 2), F(-13, 6), F(1)], m=[F(3, 2), F(-1), F(-3, 4)], v=[F(7, 4), F(7), F(7, 16)])]))

# --- where epsilon sits: the same betas, epsilon = 1e-8, gradients of 1e-6, one step.  lr_t = lr; m = g/2; sqrt(v) = |g|/2:
#   update = lr (g/2) / (|g|/2 + eps) = lr g / (|g| + 2 eps) = +- lr 1e-6 / 1.02e-6 = +- lr 50/51 = +- 25/102.
#   (torch.optim.Adam divides sqrt(v) by sqrt(1 - b2^t) = 1/2 BEFORE it adds epsilon: lr g / (|g| + eps) = lr 100/101 -- 1 % away.)
CASES.append(dict(
    name="epsilon_beside_the_uncorrected_sqrt", kw=dict(lr=F(1, 4), beta_1=F(1, 2), beta_2=F(3, 4), epsilon=F(1, 10 ** 8)),
    p0=[F(1), F(1)], grads=[[F(1, 10 ** 6), F(-1, 10 ** 6)]],
    expect=[dict(p=[F(77, 102), F(127, 102)], m=[F(1, 2 * 10 ** 6), F(-1, 2 * 10 ** 6)], v=[F(1, 4 * 10 ** 12), F(1, 4 * 10 ** 12)])]))

# --- beta_1 = 1/2, beta_2 = 0 (v = g^2, sqrt(1 - b2^t) = 1), epsilon = 1, lr = 1/2: lr_t = lr / (1 - 2^-t).
#   step 1: lr_t = 1.  g = (3, -1): m = (3/2, -1/2), v = (9, 1); update = m / (sqrt(v) + 1) = (3/8, -1/4); p = (1, -1) - . = (5/8, -3/4)
#   step 2: lr_t = (1/2) / (3/4) = 2/3.  g = (1, 3): m = (3/4 + 1/2, -1/4 + 3/2) = (5/4, 5/4), v = (1, 9);
#     update = 2/3 (5/4 / 2, 5/4 / 4) = (5/12, 5/24); p = (5/8 - 5/12, -3/4 - 5/24) = (5/24, -23/24)
_B = dict(lr=F(1, 2), beta_1=F(1, 2), beta_2=0, epsilon=1)
_B1 = dict(p=[F(5, 8), F(-3, 4)], m=[F(3, 2), F(-1, 2)], v=[F(9), F(1)])
CASES.append(dict(
    name="beta2_zero", kw=dict(_B), p0=[F(1), F(-1)], grads=[[F(3), F(-1)], [F(1), F(3)]],
    expect=[_B1, dict(p=[F(5, 24), F(-23, 24)], m=[F(5, 4), F(5, 4)], v=[F(1), F(9)])]))

# --- the same with amsgrad: vhat = max(vhat, v) = (9, 1) then (9, 9); step 2 divides by sqrt(vhat) + 1 = (4, 4):
#   update = 2/3 (5/4) / 4 = 5/24 for both; p = (5/8 - 5/24, -3/4 - 5/24) = (5/12, -23/24)
CASES.append(dict(
    name="beta2_zero_amsgrad", kw=dict(_B, amsgrad=True), p0=[F(1), F(-1)], grads=[[F(3), F(-1)], [F(1), F(3)]],
    expect=[dict(_B1, vhat=[F(9), F(1)]), dict(p=[F(5, 12), F(-23, 24)], m=[F(5, 4), F(5, 4)], v=[F(1), F(9)], vhat=[F(9), F(9)])]))

# --- the same with decay = 1: step 1 reads iterations = 0 (lr = 1/2, as above); step 2 reads iterations = 1: lr = (1/2) / (1 + 1) = 1/4,
#   lr_t = (1/4) / (3/4) = 1/3: update = 1/3 (5/4 / 2, 5/4 / 4) = (5/24, 5/48); p = (5/8 - 5/24, -3/4 - 5/48) = (5/12, -41/48)
CASES.append(dict(
    name="beta2_zero_decay", kw=dict(_B, decay=1), p0=[F(1), F(-1)], grads=[[F(3), F(-1)], [F(1), F(3)]],
    expect=[_B1, dict(p=[F(5, 12), F(-41, 48)], m=[F(5, 4), F(5, 4)], v=[F(1), F(9)])]))

# --- the same with weight_decay = 1/2, the raw gradients chosen so that g + wd p is the gradient of `beta2_zero`:
#   step 1: p = (1, -1): g = (3 - 1/2, -1 + 1/2) = (5/2, -1/2);  step 2: p = (5/8, -3/4): g = (1 - 5/16, 3 + 3/8) = (11/16, 27/8)
CASES.append(dict(
    name="beta2_zero_weight_decay", kw=dict(_B, weight_decay=F(1, 2)), p0=[F(1), F(-1)],
    grads=[[F(5, 2), F(-1, 2)], [F(11, 16), F(27, 8)]],
    expect=[_B1, dict(p=[F(5, 24), F(-23, 24)], m=[F(5, 4), F(5, 4)], v=[F(1), F(9)])]))

# Against float64 arithmetic: each expected value is reached through fewer than 20 roundings of 2^-53 relative each, and the only
# cancellation is p - update with |p| <= 4 |result|: 1e-14 relative (45 x the rounding unit) holds with room and still pins every digit
# a misplaced epsilon, a pow() instead of a product or a swapped operation order would move.
RTOL = 1e-14


def floats(xs):
    return [float(x) for x in xs]
