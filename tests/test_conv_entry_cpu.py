"""The accept / refuse decision of every convolution launch entry of libssdhip against the verdicts recorded on the commit named in
tests/conv_entry_verdicts.json: per entry a valid base call and one-at-a-time perturbations of every pointer (null, 2, 4, 8 bytes
off), dimension, channel count, kernel / stride / pad / dilation, of the form-specific arguments (pool, y2, bias_rows, oscale, ksplit
and its workspace, n_problems, variant), both sides of every reachable byte / index limit and of the map-size and width limits, and
the three host-only queries (split-K workspace bytes, the slab kernel's tiling plan, the masked form's bias rows), a few of them
under SSDHIP_CONVH_GRID=1 / SSDHIP_CONVH_STACK=0 (tests/conv_entry_cases.py).  The SSD7 family is in it too: its two convolution
entries, two pack entries and two weight gradients (element strides, workspaces, the seven geometries, the heads' row counts) and
its five queries (image bytes, the weight gradients' plans and workspace bytes).

The addresses are made up, so this runs only where no launch can succeed: there host validation is all that happens, an accepted call
ends as SSDHIP_E_LAUNCH (-3) and a refused one as SSDHIP_E_BADARG (-1) or SSDHIP_E_WORKSPACE (-2).

What it cannot see: it checks the DECISION, not the parameter struct a launcher fills -- the grid, the tile fields and the kernel
template chosen are covered by the GPU suites (tests/test_conv_gpu.py, test_forward_exact_gpu.py, test_backward_exact_gpu.py,
test_precise_gpu.py, test_train_glue_gpu.py), which compare every form's results bit for bit.  The tiling plan and the bias-row
queries do expose the slab kernel's tile fields.

`CONV_ENTRY_RECORD=<commit hash> pytest tests/test_conv_entry_cpu.py` writes the verdicts instead of comparing against them."""
import json
import os

import pytest

from . import conv_entry_cases as cec


@pytest.fixture(scope="module")
def recorded():
    import torch
    if torch.cuda.is_available():
        pytest.skip("made-up device addresses: only where no launch can succeed")
    commit = os.environ.get(cec.RECORD_ENV)
    if commit:
        cec.write_verdicts(commit)
    with open(cec.VERDICTS) as f:
        return json.load(f)


def test_verdicts_cover_every_case(recorded):
    assert sorted(recorded["verdicts"]) == sorted(cec.cases()) and sorted(recorded["queries"]) == sorted(cec.queries())
    assert len(recorded["recorded_on_commit"]) == 40
    assert len(recorded["verdicts"]) >= 300
    # every entry's base call is accepted, and every entry has refused cases
    for entry in cec.ENTRIES:
        assert recorded["verdicts"][entry + "|"] == -3, entry
        assert any(v == -1 for k, v in recorded["verdicts"].items() if k.startswith(entry + "|")), entry
    assert -2 in recorded["verdicts"].values()


@pytest.mark.parametrize("entry", sorted(cec.ENTRIES))
def test_entry_decisions_match_recorded_verdicts(recorded, entry):
    lib = cec.nat.load()
    wrong, n = [], 0
    for cid, case in cec.cases().items():
        if case[0] != entry:
            continue
        got, want = cec.run_case(lib, *case), recorded["verdicts"][cid]
        n += 1
        if got != want:
            wrong.append((cid, want, got))
    assert n and not wrong, "%d of %d cases differ from the recorded verdicts (case, recorded, now):\n%s" % (
        len(wrong), n, "\n".join(map(str, wrong[:10])))


def test_host_queries_match_recorded_values(recorded):
    lib = cec.nat.load()
    wrong = [(qid, recorded["queries"][qid], got) for qid, q in cec.queries().items()
             for got in [cec.run_query(lib, *q)] if got != recorded["queries"][qid]]
    assert not wrong, "%d queries differ from the recorded values (query, recorded, now):\n%s" % (
        len(wrong), "\n".join(map(str, wrong[:10])))
