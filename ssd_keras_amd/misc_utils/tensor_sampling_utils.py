"""`sample_tensors` -- drop-in for the reference's misc_utils/tensor_sampling_utils.py:21-177 (weight_sampling_tutorial.ipynb): sub- and
up-sample corresponding axes of a list of weight tensors, the way the tutorial cuts a trained classifier down to (or pads it up to)
another number of classes.

Two forms, one selection.  NumPy arrays in: the list the reference returns, bit for bit -- sub-sampled tensors keep their dtype,
up-sampled ones come back float64 (the fill is float64 and the originals are scattered into it) -- with the global `np.random` stream
consumed call for call as there: per sub-sampled integer axis one `choice` without replacement over 1 .. n-1 (sorted; index 0, the
background class, is always kept), then, when any axis grows, the first tensor's `normal` fill, one `choice` per growing axis for the
scatter positions, and the further tensors' fills in list order ('zeros' draws nothing).  torch tensors in (CPU or CUDA): the same
selection and the same draws on the host, the gathers and scatters on the tensors' device, results in each input's dtype; the float64
fill is rounded to that dtype once.

Mirrored as found rather than repaired: index lists are checked against the axis length from above only (negative indices wrap as
NumPy's do); `int` is tested with isinstance, so a NumPy integer is refused and a bool counts as 0 / 1; an unknown `init` string is
only noticed when something is up-sampled, after the draws in front of it.
"""
import numpy as np
import torch


def _plan(shape, sampling_instructions):
    """Per axis of the first tensor: the indices to gather (consuming `np.random` for integer sub-sampling), the length asked for, and
    the axes that grow."""
    picks, lengths, growing = [], [], []
    for axis, inst in enumerate(sampling_instructions):
        n = shape[axis]
        if isinstance(inst, (list, tuple)):
            top = np.amax(np.array(inst))
            if top >= n:
                raise ValueError("The sampling instructions for axis {} contain index {}, but that axis has only {} elements."
                                 .format(axis, top, n))
            picks.append(np.array(inst))
            lengths.append(len(inst))
        elif isinstance(inst, int):
            lengths.append(inst)
            if inst < n:
                rest = np.sort(np.random.choice(np.arange(1, n), inst - 1, replace=False))
                picks.append(np.concatenate([np.array([0]), rest]))
            else:
                picks.append(np.arange(n))
                if inst > n:
                    growing.append(axis)
        else:
            raise ValueError("A sampling instruction is an int or a list / tuple of ints, got `{}` for axis {}.".format(type(inst), axis))
    return picks, lengths, growing


def _gather(t, index_arrays):
    grid = np.ix_(*index_arrays)
    if torch.is_tensor(t):
        return t[tuple(torch.from_numpy(np.ascontiguousarray(g)).to(t.device) for g in grid)]
    return np.copy(t[grid])


def _fill(like, how, size, mean, stddev):
    """The tensor the originals are scattered into: a float64 draw (or zeros) on the host; for a torch input rounded once to its dtype."""
    if how is None or how == 'gaussian':
        full = np.random.normal(loc=mean, scale=stddev, size=size)
    elif how == 'zeros':
        full = np.zeros(size)
    else:
        raise ValueError("`init` entries are 'gaussian' or 'zeros', got '{}'.".format(how))
    if torch.is_tensor(like):
        return torch.from_numpy(np.ascontiguousarray(full)).to(like.dtype).to(like.device)
    return full


def _scatter(full, index_arrays, values):
    grid = np.ix_(*index_arrays)
    if torch.is_tensor(full):
        grid = tuple(torch.from_numpy(np.ascontiguousarray(g)).to(full.device) for g in grid)
    full[grid] = values
    return full


def sample_tensors(weights_list, sampling_instructions, axes=None, init=None, mean=0.0, stddev=0.005):
    """Sub- and / or up-sample axes of the tensors in `weights_list` consistently.

    weights_list: NumPy arrays, or torch tensors (not both); the first has the most axes (a convolution's kernel before its bias).
    sampling_instructions: one entry per axis of the first tensor -- a list / tuple of indices to keep, or an int: the new length
        (smaller: random sub-sampling that always keeps index 0; equal: unchanged; larger: the old entries are spread over random
        positions, index 0 staying first, and the gaps filled).
    axes: for each further tensor, the axes of the first tensor its own axes correspond to (`[[3]]` for a Conv2D bias).
    init: None (all 'gaussian') or one of 'gaussian' / 'zeros' per tensor: what fills the gaps of an up-sampled axis.
    mean, stddev: of the Gaussian fill.
    Returns the list of sampled tensors, in order."""
    tensor_form = {bool(torch.is_tensor(w)) for w in weights_list}
    if len(tensor_form) > 1:
        raise TypeError("`weights_list` mixes NumPy arrays and torch tensors; pass one kind.")
    first = weights_list[0]
    if not isinstance(sampling_instructions, (list, tuple)) or len(sampling_instructions) != first.ndim:
        raise ValueError("`sampling_instructions` must be a list with one entry per axis of the first tensor in `weights_list`.")
    if init is not None and len(init) != len(weights_list):
        raise ValueError("`init` must be None or hold one string per tensor in `weights_list`.")

    picks, lengths, growing = _plan(tuple(first.shape), sampling_instructions)
    sampled = [_gather(first, picks)]
    for j in range(1, len(weights_list)):
        sampled.append(_gather(weights_list[j], [picks[i] for i in axes[j - 1]]))
    if not growing:
        return sampled

    lengths = np.array(lengths)
    full = _fill(first, None if init is None else init[0], lengths, mean, stddev)
    places = [np.arange(k) for k in sampled[0].shape]
    for axis in growing:
        rest = np.sort(np.random.choice(np.arange(1, full.shape[axis]), sampled[0].shape[axis] - 1, replace=False))
        places[axis] = np.concatenate([np.array([0]), rest])
    out = [_scatter(full, places, sampled[0])]
    for j in range(1, len(weights_list)):
        full = _fill(weights_list[j], None if init is None else init[j], lengths[axes[j - 1]], mean, stddev)
        out.append(_scatter(full, [places[i] for i in axes[j - 1]], sampled[j]))
    return out
