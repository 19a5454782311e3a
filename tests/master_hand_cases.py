"""float32 master weights behind bf16 parameters (`master_weights=True` of ssd_keras_amd.optimizers): cases worked out BY HAND in exact
fractions, shared by the CPU tests (the tensor expressions) and the GPU tests (ssdhip_sgd_step_bf16 / ssdhip_adam_step_bf16).

bf16 keeps 8 significant bits: its values are 2^-8 apart in [1/2, 1), 2^-7 apart in [1, 2) and 2^-9 apart in [1/4, 1/2).  A master is
rounded to the nearest of them, a tie to the one whose last bit is 0.

--- SGD(lr = 2^-12, momentum = 1/2, rule = 'keras'), gradient 1 at every step, parameters (1, -1, 1/2).
    v_k = v_{k-1} / 2 - 2^-12  =  -2^-11 (1 - 2^-k)                      (v_0 = 0)
    w_k = w_{k-1} + v_k        =  w_0 - 2^-11 (k - 1 + 2^-k)
  Every value is dyadic and needs bits down to 2^-(11+k) only: float32 holds them exactly for k <= 12 (ulp 2^-24 below 1, 2^-23 above
  1, 2^-25 below 1/2), so the master is asserted EXACTLY.  Write d_k = k - 1 + 2^-k (so w_k = w_0 - 2^-11 d_k): d = 0.5, 1.25, 2.125,
  3.0625, 4.03, 5.02, 6.01, 7.004, 8.002, 9.001, 10.0005, 11.0002 for k = 1 .. 12.
    w_0 = 1:    the midpoint below 1 is 1 - 2^-9 = 1 - 2^-11 * 4 (a tie would go to 1, whose last bit is 0): p = 1 while d_k <= 4,
                i.e. k <= 4; p = 1 - 2^-8 from k = 5 (the next midpoint, 1 - 2^-11 * 12, is not reached in 12 steps).
    w_0 = -1:   the values beyond -1 are 2^-7 apart, the midpoint is -(1 + 2^-8) = -1 - 2^-11 * 8: p = -1 for k <= 8 (d_8 = 7.004),
                p = -(1 + 2^-7) from k = 9 (d_9 = 8.002; the next midpoint is at d = 24).
    w_0 = 1/2:  the values below 1/2 are 2^-9 apart, the midpoints at d = 2, 6, 10, 14: p = 1/2 for k <= 2 (d_2 = 1.25),
                1/2 - 2^-9 for k = 3 .. 6 (d_6 = 5.02), 1/2 - 2^-8 for k = 7 .. 10 (d_7 = 6.01, d_10 = 9.001), 1/2 - 3 * 2^-9 for k = 11, 12.
  Without masters the same run never moves: the velocity settles near -2^-11, and 1 - 2^-11, -1 - 2^-11 and 1/2 - 2^-11 all lie within
  half a step of the value they started from.

--- Adam(lr = 5 * 2^-14, epsilon = 0), gradient 1 at every step, parameters (1, -1, 1/2).
    m_k = (1 - b1^k) g, v_k = (1 - b2^k) g^2, lr_t = lr sqrt(1 - b2^k) / (1 - b1^k):  lr_t m_k / sqrt(v_k) = lr sign(g) = lr
    w_k = w_0 - k lr = w_0 - 2^-14 * 5 k                                 (up to float32 rounding: asserted to 1e-6 relative)
  lr is chosen so that no step lands on or near a midpoint (the nearest miss is a fifth of a step, 6e-5: sixty times the tolerance):
    w_0 = 1:    midpoints at 2^-9 = 2^-14 * 32 and 2^-14 * 96: p = 1 for 5 k < 32, i.e. k <= 6; 1 - 2^-8 for k = 7 .. 14.
    w_0 = -1:   midpoint at 2^-8 = 2^-14 * 64: p = -1 for k <= 12; -(1 + 2^-7) for k = 13, 14.
    w_0 = 1/2:  midpoints at 2^-14 * 16, 48, 80: p = 1/2 for k <= 3; 1/2 - 2^-9 for k = 4 .. 9; 1/2 - 2^-8 for k = 10 .. 14."""
from fractions import Fraction as F

import numpy as np

P0 = [F(1), F(-1), F(1, 2)]
GRAD = [F(1), F(1), F(1)]


def _table(changes, steps):
    """[(first step, value), ...] -> the value at steps 1 .. steps."""
    out = []
    for k in range(1, steps + 1):
        out.append([v for first, v in changes if first <= k][-1])
    return out


SGD_KW = dict(lr=F(1, 2 ** 12), momentum=F(1, 2), rule="keras")
SGD_STEPS = 12
SGD_P = [_table([(1, F(1)), (5, 1 - F(1, 2 ** 8))], SGD_STEPS),
         _table([(1, F(-1)), (9, -(1 + F(1, 2 ** 7)))], SGD_STEPS),
         _table([(1, F(1, 2)), (3, F(1, 2) - F(1, 2 ** 9)), (7, F(1, 2) - F(1, 2 ** 8)), (11, F(1, 2) - F(3, 2 ** 9))], SGD_STEPS)]
SGD_FIRST_MOVE = [5, 9, 3]                                 # the step at which each value's bf16 parameter first differs from p0


def sgd_velocity(k):
    return -F(1, 2 ** 11) * (1 - F(1, 2 ** k))


def sgd_master(w0, k):
    return w0 - F(1, 2 ** 11) * (k - 1 + F(1, 2 ** k))


ADAM_KW = dict(lr=F(5, 2 ** 14), beta_1=F(9, 10), beta_2=F(999, 1000), epsilon=0)
ADAM_STEPS = 14
ADAM_P = [_table([(1, F(1)), (7, 1 - F(1, 2 ** 8))], ADAM_STEPS),
          _table([(1, F(-1)), (13, -(1 + F(1, 2 ** 7)))], ADAM_STEPS),
          _table([(1, F(1, 2)), (4, F(1, 2) - F(1, 2 ** 9)), (10, F(1, 2) - F(1, 2 ** 8))], ADAM_STEPS)]
ADAM_RTOL = 1e-6                                           # as tests/test_optim_gpu.py: a handful of float32 roundings of 6e-8 each


def adam_master(w0, k):
    return w0 - k * ADAM_KW["lr"]


def floats(xs):
    return [float(x) for x in xs]


def kwargs(kw):
    return {k: (v if isinstance(v, (str, bool)) else float(v)) for k, v in kw.items()}


# ---- bf16 in NumPy: bits as uint16 ----------------------------------------------------------------------------------------------
def bf16_round_bits(x):
    """float32 array -> the bits (uint16) of the nearest bf16 value, ties to even (finite values)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


def bf16_bits_to_float32(b):
    return (np.ascontiguousarray(b).astype(np.uint32) << np.uint32(16)).view(np.float32)


def bits_of(t):
    """A bf16 torch tensor's bits as a uint16 array in the tensor's logical order."""
    import torch
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)
