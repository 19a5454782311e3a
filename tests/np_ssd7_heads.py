"""Float64 NumPy statement of the packed predictor heads of SSD7's training step (csrc/ssdhip_heads7.hip): the conf and loc heads of a
source map, two Conv2D(3 x 3, 'same') on the same input, as ONE convolution whose filters are [conf | loc | zero rows] up to 48 output
channels -- forward, data gradient and the four parameter gradients -- on tests/np_ssd7_conv.py's shifted multiply-adds.  Maps are NHWC
arrays [B, H, W, C], filters [n, 3, 3, Cin].  tests/test_ssd7_head_reference_cpu.py pins this module to torch's CPU float64 autograd of
the two separate convolutions."""
import numpy as np

from tests import np_ssd7_conv as conv

CP = 48
# (Cin, (H, W)) of the four source maps for the 300 x 300 and the 300 x 480 images of ssd7_training.ipynb
SOURCES = (64, 48, 48, 32)
MAPS_300x300 = [(37, 37), (18, 18), (9, 9), (4, 4)]
MAPS_300x480 = [(37, 60), (18, 30), (9, 15), (4, 7)]



def _kernel_cases():
    """(Cin, B, H, W, n_conf, n_loc) of tests/test_ssd7_head_kernels_gpu.py: every map size with every Cin; the batch (1, 3) and the packed
    width -- 40 = 4 boxes x (6 + 4), 30 = 3 boxes x (6 + 4), 48 = 4 boxes x (8 + 4), no padding rows -- cycle through the list so that
    each batch and each width meets every Cin and several map sizes."""
    maps, widths = [(1, 1), (2, 2), (4, 4), (9, 8), (5, 3)], [(24, 16), (18, 12), (32, 16)]
    cases = []
    for h, w in maps:
        for cin in (64, 48, 32):
            i = len(cases)
            cases.append((cin, (1, 3)[i % 2], h, w) + widths[(i // 3 + i) % 3])
    return cases


KERNEL_CASES = _kernel_cases()
# 3 x 28 x 27 = 2268 list positions = 9 chunks of 256: five splits of two chunks, the last of one (checked against the plan)
SPLIT_CASES = [(32, 3, 26, 25, 24, 16), (64, 3, 26, 25, 18, 12)]


def packed_filters(wc, wl, cp=CP):
    """[conf | loc | zero rows]: [cp, 3, 3, Cin]."""
    wc, wl = np.asarray(wc, dtype=np.float64), np.asarray(wl, dtype=np.float64)
    assert wc.shape[1:] == wl.shape[1:] and wc.shape[0] + wl.shape[0] <= cp
    return np.concatenate([wc, wl, np.zeros((cp - wc.shape[0] - wl.shape[0],) + wc.shape[1:])], axis=0)


def packed_bias(bc, bl, cp=CP):
    bc, bl = np.asarray(bc, dtype=np.float64), np.asarray(bl, dtype=np.float64)
    return np.concatenate([bc, bl, np.zeros(cp - bc.size - bl.size)])


def forward(x, wc, bc, wl, bl, cp=CP):
    """The packed map [B, H, W, cp]: channels [conf head | loc head | zeros]."""
    return conv.conv_same(x, packed_filters(wc, wl, cp), packed_bias(bc, bl, cp))


def input_grad(dy, wc, wl):
    """dL/dx [B, H, W, Cin] from the packed dL/dy [B, H, W, cp]: both heads' contributions; the padding channels of dy meet zero filters."""
    return conv.conv_same_input_grad(dy, packed_filters(wc, wl, np.asarray(dy).shape[3]))


def param_grads(x, dy, n_conf, n_loc):
    """(dw_conf [n_conf, 3, 3, Cin], db_conf, dw_loc [n_loc, 3, 3, Cin], db_loc) from the packed dL/dy: the rows of the packed
    convolution's gradient, the padding rows dropped."""
    dw, db = conv.conv_same_weight_grad(x, dy, 3)
    return dw[:n_conf], db[:n_conf], dw[n_conf:n_conf + n_loc], db[n_conf:n_conf + n_loc]


def padded_list_positions(b, h, w):
    """Positions of the list the weight-gradient kernel walks: every image as (h + 2) x (w + 2) with a zero border, image after image."""
    return b * (h + 2) * (w + 2)
