"""Gradient clipping without a GPU: the NumPy restatement (tests/np_clip.py) against the cases worked by hand
(tests/clip_hand_cases.py), the constructors' new keywords and their errors, that the pinned parameter lists did not grow, that the
settings travel with state_dict and pickle, and that the new exports are declared once in the header and in the ctypes table."""
import copy
import inspect
import os
import pickle
import re

import numpy as np
import pytest

from tests import clip_hand_cases as hand
from tests import np_clip, np_sgd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ["ssdhip_clip_state_bytes", "ssdhip_clip_state_init", "ssdhip_grad_sumsq_partials", "ssdhip_clip_finish",
               "ssdhip_sgd_step_clipped", "ssdhip_sgd_step_bf16_clipped", "ssdhip_adam_step_clipped", "ssdhip_adam_step_bf16_clipped"]


@pytest.mark.parametrize("case", hand.CASES, ids=[c["name"] for c in hand.CASES])
def test_restatement_on_the_hand_cases(case):
    """SGD, rule 'torch', lr 1, momentum 1/2 from a zero buffer: buf = out and p = w - out, both exact."""
    clip = np_clip.Clip(case["clipnorm"], case["clipvalue"], case["skip_nonfinite"])
    rule = np_sgd.SGD(lr=1.0, momentum=0.5)
    t = np_sgd.fresh(case["w"])
    out = np_clip.step(clip, [dict(rule=rule, wd=case["weight_decay"], tensors=[t], grads=[case["g"]], vector=4)])
    assert hand.same(clip.q, case["q"]) and hand.same(clip.norm, case["norm"]) and hand.same(clip.scale, case["scale"])
    assert clip.stats == {"steps": 1, "clipped": int(case["clipped"]), "skipped": int(case["skipped"])}
    if case["out"] is None:
        assert out is None and rule.iterations == 0
        assert t["p"].tobytes() == case["w"].tobytes() and not t["buf"].any()
    else:
        assert hand.same(out[0][0], case["out"]) and rule.iterations == 1
        assert hand.same(t["buf"], case["out"]) and hand.same(t["p"], case["w"] - case["out"])


def test_the_norm_is_one_norm_over_every_tensor_of_every_group():
    clip = np_clip.Clip(clipnorm=6.5)
    groups = [dict(rule=np_sgd.SGD(lr=1.0, momentum=0.5), wd=0.0, tensors=[np_sgd.fresh(np.zeros(1, np.float32))],
                   grads=[np.array([x], np.float32)], vector=v) for x, v in ((3.0, 4), (4.0, 8), (12.0, 4))]
    out = np_clip.step(clip, groups)
    assert clip.q == 169.0 and clip.norm == 13.0 and clip.scale == 0.5
    assert [float(o[0][0]) for o in out] == [1.5, 2.0, 6.0]


def _optimizers():
    from ssd_keras_amd.optimizers import SGD, Adam
    return SGD, Adam


def _params(n=2):
    import torch
    return [torch.nn.Parameter(torch.zeros(3)) for _ in range(n)]


def test_the_keywords_exist_and_the_pinned_parameter_lists_did_not_grow():
    SGD, Adam = _optimizers()
    assert list(inspect.signature(SGD.__init__).parameters)[1:] == ["params", "lr", "momentum", "weight_decay", "decay", "nesterov", "rule"]
    assert list(inspect.signature(Adam.__init__).parameters)[1:] == ["params", "lr", "beta_1", "beta_2", "epsilon", "decay", "amsgrad",
                                                                     "weight_decay"]
    for cls, kw in ((SGD, dict(momentum=0.9)), (Adam, {})):
        plain = cls(_params(), **kw)
        assert plain._clip() is None
        assert all((g["clipnorm"], g["clipvalue"], g["skip_nonfinite"]) == (None, None, False) for g in plain.param_groups)
        assert plain.grad_norm is None and plain.clip_stats == {"steps": 0, "clipped": 0, "skipped": 0}
        opt = cls(_params(), clipnorm=2.5, clipvalue=0.5, skip_nonfinite=True, master_weights=True, **kw)
        assert opt._clip() == (2.5, 0.5, True)
        assert all((g["clipnorm"], g["clipvalue"], g["skip_nonfinite"], g["master_weights"]) == (2.5, 0.5, True, True)
                   for g in opt.param_groups)
        assert cls(_params(), clipnorm=1.0, **kw)._clip() == (1.0, 0.0, False)
        assert cls(_params(), skip_nonfinite=True, **kw)._clip() == (0.0, 0.0, True)
        assert cls(_params(), clipnorm=0.0, clipvalue=0, **kw)._clip() is None        # Keras: a bound applies when it is > 0


def test_constructor_errors():
    SGD, Adam = _optimizers()
    for cls, kw in ((SGD, dict(momentum=0.9)), (Adam, {})):
        for bad in (dict(clipnorm=-1.0), dict(clipvalue=-0.5), dict(clipnorm=float("nan"))):
            with pytest.raises(ValueError):
                cls(_params(), **bad, **kw)
        a, b = _params(1), _params(1)
        with pytest.raises(ValueError, match="optimizer-wide"):                       # groups that disagree
            cls([dict(params=a), dict(params=b, clipnorm=2.0)], clipnorm=1.0, **kw)
        with pytest.raises(ValueError, match="optimizer-wide"):
            cls([dict(params=a), dict(params=b, skip_nonfinite=True)], **kw)
        opt = cls(a, clipnorm=1.0, **kw)
        with pytest.raises(ValueError, match="optimizer-wide"):
            opt.add_param_group(dict(params=b, clipnorm=3.0))
        cls([dict(params=a), dict(params=b, clipnorm=1.0)], clipnorm=1.0, **kw)       # groups that agree are fine


def test_a_parameter_off_the_fused_launch_is_refused_by_name_before_anything_happens():
    """CPU parameters go through the tensor expressions, which do not clip: refused, and nothing has moved."""
    import torch
    SGD, Adam = _optimizers()
    for cls, kw in ((SGD, dict(momentum=0.9)), (Adam, {})):
        ps = _params(3)
        ps[0].grad = None
        for p in ps[1:]:
            p.grad = torch.ones(3)
        opt = cls(ps, clipnorm=1.0, **kw)
        for call in (opt.step, opt.init_state):
            with pytest.raises(ValueError, match="parameter 1 of group 0"):
                call()
        assert not opt.state and all(not p.detach().any() for p in ps)
        plain = cls(ps, **kw)                                                     # the same parameters without clipping: a step
        plain.step()
        assert ps[1].detach().abs().sum() > 0


def test_settings_travel_with_state_dict_pickle_and_deepcopy():
    SGD, Adam = _optimizers()
    for cls, kw in ((SGD, dict(momentum=0.9)), (Adam, {})):
        opt = cls(_params(), clipnorm=2.5, clipvalue=0.25, skip_nonfinite=True, **kw)
        sd = opt.state_dict()
        assert (sd["param_groups"][0]["clipnorm"], sd["param_groups"][0]["clipvalue"], sd["param_groups"][0]["skip_nonfinite"]) == (2.5, 0.25, True)
        other = cls(_params(), **kw)
        other.load_state_dict(sd)
        assert other._clip() == (2.5, 0.25, True)
        assert pickle.loads(pickle.dumps(opt))._clip() == (2.5, 0.25, True)
        assert copy.deepcopy(opt)._clip() == (2.5, 0.25, True)
        old = cls(_params(), **kw).state_dict()                                   # a checkpoint from before the keywords existed
        for g in old["param_groups"]:
            for k in ("clipnorm", "clipvalue", "skip_nonfinite"):
                del g[k]
        restored = cls(_params(), **kw)
        restored.load_state_dict(old)
        assert restored._clip() is None and restored.param_groups[0]["clipnorm"] is None


def test_new_exports_are_declared_once_in_the_header_and_in_the_ctypes_table():
    from ssd_keras_amd import _native as nat
    hdr = open(os.path.join(ROOT, "include", "ssdhip.h")).read()
    code = re.sub(r"/\*.*?\*/|//[^\n]*", " ", hdr, flags=re.S)
    src = open(os.path.join(ROOT, "ssd_keras_amd", "_native.py")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW_EXPORTS:
        assert len(re.findall(r"\b%s\s*\(" % name, code)) == 1, name
        assert name in nat.SIGNATURES and src.count('"%s":' % name) == 1, name
        assert name in doc, name
    assert "typedef struct ssdhip_clip_state {" in code
    # the record the host reads a block with is the struct: 64 bytes, a multiple of the 16-byte alignment
    assert nat.CLIP_STATE.itemsize == 64
    assert nat.CLIP_STATE.names == ("q", "steps", "clipped", "skipped", "clipnorm", "clipvalue", "norm", "scale", "skip_nonfinite", "skip",
                                    "reserved")
    assert nat.ABI_VERSION == 1
