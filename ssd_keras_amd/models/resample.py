"""`resample_classes` -- the reference's weight_sampling_tutorial.ipynb on a LIVE model: a new SSD300 / SSD512 / SSD7 for another set of
classes whose classifier heads are `sample_tensors` of the given model's, everything else equal.

No kernel was added for this: it runs once per fine-tuning job over a few megabytes of classifier weights (index gathers on the
parameters' device).  What matters on the device is what the model derives from its parameters -- packed head images, bf16 shadows,
BatchNorm tables, captured graphs, optimizer masters: the result is a freshly constructed model, so it holds none of them, and
`fused_blocks(...)`, `precise()`, `graphed(...)` and the optimizer are set up again on it.
"""
from __future__ import annotations

import copy

import torch

from ..misc_utils.tensor_sampling_utils import sample_tensors
from .keras_weights import keras_layer_map


def _like(new, old):
    """`new` in `old`'s dtype and memory format (a channels_last model keeps channels_last filters)."""
    new = new.to(old.dtype)
    if new.dim() == 4 and old.is_contiguous(memory_format=torch.channels_last) and not old.is_contiguous():
        return new.contiguous(memory_format=torch.channels_last)
    return new.contiguous()


def resample_classes(model, classes_of_interest, init=('gaussian', 'zeros'), mean=0.0, stddev=0.005):
    """A NEW model of `model`'s class and configuration -- device, dtype, memory format and train() / eval() mode included -- for the
    classes `classes_of_interest`; `model` itself is left untouched.

    classes_of_interest: a list of `model`'s class indices in the order the new model numbers them (0, the background, first, as in
        the tutorial): the new model has `len(classes) - 1` object classes; or an int, the new number of classes with the background:
        random sub-sampling, or up-sampling with the gaps filled per `init` (kernel, bias) / `mean` / `stddev`.
    Every parameter and buffer equals `model`'s except the conf heads, which are
    `sample_tensors([kernel, bias], [kh, kw, in, .], axes=[[3]], ...)` of `model`'s in head order, gathered on the parameters' device
    and consuming the global `np.random` stream as the file route does.  The function sees what `resample_keras_weights` sees in a
    file of the model -- the heads in Keras' HWIO layout (through `keras_layer_map`'s converters), 16-bit parameters widened to the
    file's float32 and the result cast back as `load_keras_weights` casts it -- so under the same `np.random` state the two routes
    give equal parameters, for bf16 models too (a Gaussian fill is rounded float64 -> float32 -> bf16 on both; a float64 model keeps
    float64 throughout, which a weight file would not).
    The new model's switches (`fused_blocks`, `precise`, `graphed`, `fused_inference` / `fused_training`) start at their defaults and
    nothing derived from `model`'s weights is copied; `l2_regularization` and the input normalisation attributes are taken as
    `model` has them now.  Constructing it draws the usual initial weights from torch's generator."""
    config = getattr(model, "_init_config", None)
    if config is None:
        raise TypeError("resample_classes needs an SSD300 / SSD512 / SSD7 of this package, got {}".format(type(model).__name__))
    n_source = model.n_classes                                   # with the background
    if isinstance(classes_of_interest, int):
        n_new = classes_of_interest
    else:
        classes_of_interest = list(classes_of_interest)
        n_new = len(classes_of_interest)
    if n_new < 2:
        raise ValueError("the new model needs the background and at least one class, got {}".format(n_new))
    new = type(model)(**dict(config, n_classes=n_new - 1))
    for name in ("l2_regularization", "subtract_mean", "divide_by_stddev", "swap_channels"):
        setattr(new, name, copy.deepcopy(getattr(model, name)))              # plain attributes a caller may have set since construction
    ref = next(model.parameters())
    new.to(device=ref.device, dtype=ref.dtype)

    old_map, new_map = keras_layer_map(model), keras_layer_map(new)
    conf_names = [name for name, items in old_map.items() if any(items[0][0] is ch.weight for ch in model.conf_heads)]
    assert len(conf_names) == len(model.conf_heads)
    resampled = {}
    with torch.no_grad():
        for name in conf_names:
            (w, _, w_to_keras), (b, _, b_to_keras) = old_map[name]
            wide = lambda t: t.detach().float() if t.dtype in (torch.bfloat16, torch.float16) else t.detach()
            kernel, bias = w_to_keras(wide(w)), b_to_keras(wide(b))
            kh, kw, cin, cout = kernel.shape
            n_boxes = cout // n_source
            if isinstance(classes_of_interest, int):
                last = int(classes_of_interest * cout / n_source)
            else:
                last = [c + i * n_source for i in range(n_boxes) for c in classes_of_interest]
            out = sample_tensors([kernel, bias], [kh, kw, cin, last], axes=[[3]], init=init, mean=mean, stddev=stddev)
            for (t_new, to_torch, _), o, t_old in zip(new_map[name], out, (w, b)):
                resampled[id(t_new)] = _like(to_torch(o), t_old)
                if resampled[id(t_new)].shape != t_new.shape:
                    raise ValueError("layer '{}': the resampled shape {} does not fit the new model's {}".format(
                        name, tuple(resampled[id(t_new)].shape), tuple(t_new.shape)))
        old_state = dict(list(model.named_parameters()) + list(model.named_buffers()))
        for key, t_new in list(new.named_parameters()) + list(new.named_buffers()):
            t_old = old_state[key]
            t_new.data = resampled[id(t_new)] if id(t_new) in resampled else t_old.detach().clone(memory_format=torch.preserve_format)
        for key, p_new in new.named_parameters():
            p_new.requires_grad_(old_state[key].requires_grad)
    for m_old, m_new in zip(model.modules(), new.modules()):
        m_new.training = m_old.training
    return new
