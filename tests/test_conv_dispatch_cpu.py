"""The per-layer kernel selection of ssd_keras_amd.models against the trace recorded on the commit named in
tests/conv_dispatch_trace.json: the candidates offered and their order, the autotune keys, the forms taken without a timing run and
every libssdhip call with its arguments, for every convolution geometry of SSD300 / SSD512 at batch 1, 8, 16 and 32 under the default
environment and under each selection switch alone (tests/conv_dispatch_cases.py).  Needs no GPU.

`CONV_DISPATCH_RECORD=<commit hash> pytest tests/test_conv_dispatch_cpu.py` writes the trace instead of comparing against it."""
import json
import os

import pytest

from . import conv_dispatch_cases as cdc


@pytest.fixture(scope="module")
def recorded():
    commit = os.environ.get(cdc.RECORD_ENV)
    if commit:
        cdc.write_trace(commit)
    with open(cdc.TRACE) as f:
        return json.load(f)


def test_trace_covers_every_case(recorded):
    assert recorded["environments"] == [e or "default" for e in cdc.ENVS] and recorded["batches"] == list(cdc.BATCHES)
    assert sorted(recorded["cases"]) == sorted(cdc.case_ids())
    assert len(recorded["recorded_on_commit"]) == 40


def test_link_out_on_a_layer_without_relu_is_refused():
    """The consumer of a link masks its data gradient by this layer's output > 0: only the ReLU backward of a ReLU layer is that mask."""
    model, conv = cdc.Tracer().model, cdc.nn.Conv2d(8, 8, 3, padding=1)
    x = cdc.torch.zeros(1, 8, 4, 4)
    with cdc.torch.enable_grad():
        link = model.relu_link()
        assert link is not None
        with pytest.raises(ValueError, match="link_out"):
            model.conv_act(conv, x, relu=False, link_out=link)
        assert model.conv_act(conv, x, relu=True, link_out=link).shape == (1, 8, 4, 4)
        assert model.conv_act(conv, x, relu=False).shape == (1, 8, 4, 4)


@pytest.mark.parametrize("entry", cdc.ENTRIES + ("conv1_block",))
def test_dispatch_matches_recorded_trace(recorded, entry):
    wrong, n = [], 0
    with cdc.Tracer().patched() as tracer, cdc.torch.no_grad():
        for cid in recorded["cases"]:
            if cid.split("|")[0] != entry:
                continue
            for batch in cdc.BATCHES:
                got = cdc.run_case(tracer, cid, batch)
                for env in cdc.ENVS:
                    # (an environment the case did not run under: it never reads that variable, so its outcome there is the default one)
                    want = cdc.recorded_outcome(recorded, cid, batch, env)
                    n += 1
                    if got.get(env, got[None]) != want:
                        wrong.append(("%s at batch %d under %s" % (cid, batch, env or "the default environment"), want, got.get(env, got[None])))
    assert n and not wrong, "%d of %d cases differ from the recorded trace; the first:\n%s\nrecorded: %s\nnow:      %s" % (
        (len(wrong), n) + tuple(json.dumps(v) for v in (wrong[0] if wrong else ("", "", ""))))
