"""The loss case table (tests/loss_cases.py) against the oracle and `ssdhip_loss_plan` alone, no GPU: the table reaches every kernel
path the launchers can choose, no level case has two losses close enough for a device logf to reorder them, and every select
case is what its name says.  A later change of the plan that moves a case to another path fails here, not silently."""
import numpy as np
import pytest

from tests import loss_cases as lc


@pytest.fixture(scope="module")
def lib():
    from ssd_keras_amd import _native as nat
    from ssd_keras_amd import build
    assert build.build() == nat.lib_path()
    return nat.load()


def _plans(lib):
    plans = {c.name: lc.plan(lib, c) for c in lc.ALL}
    for c, ot, op in lc.MISALIGNED:
        plans["%s+%d+%d" % (c.name, ot, op)] = lc.plan(lib, c, y_true=ot, y_pred=op)
    plans["mixed"] = lc.plan(lib, lc.PATH[4], grad=4)
    return plans


def test_case_shapes_are_the_issue_table():
    assert [c.shape for c in lc.PATH] == [(1, 4, 2), (1, 64, 2), (2, 37, 2), (3, 341, 5), (2, 68, 4), (2, 60, 7), (70, 12, 3),
                                          (2, 132, 24), (2, 132, 25), (2, 130, 21)]
    assert [c.shape for c in lc.WIDE] == [(2, 70, 116), (1, 70, 250)]
    assert all(c.shape == (3, 180001, 2) for c in lc.ALL_TIES + [lc.INTERLEAVED])
    assert [c.kw["n_neg_min"] for c in lc.ALL_TIES] == [1, 7, 8, 9, 2047, 2048, 2049, 524287, 524288, 524289, 540002, 540003]
    assert lc.LEVEL3.shape == lc.LEVEL2.shape == (2, 6148, 2) and lc.UNNORMALISED.shape == (3, 4099, 2)


def test_every_path_is_hit(lib, monkeypatch):
    monkeypatch.delenv("SSDHIP_LOSS_STREAM", raising=False)
    plans = _plans(lib)
    by = lambda f: sorted(n for n, p in plans.items() if f(p))
    assert by(lambda p: p["fwd_stream"] and p["bwd_stream"]) and by(lambda p: not p["fwd_stream"] and not p["bwd_stream"])
    assert by(lambda p: p["fwd_stream"] and not p["bwd_stream"]) == ["mixed"]
    assert not by(lambda p: p["bwd_stream"] and not p["fwd_stream"])
    tiled = [p for p in plans.values() if not p["fwd_stream"]]
    assert {p["TA"] for p in tiled} == {256, 128, 64}
    assert {p["G"] for p in plans.values() if p["fwd_stream"]} >= {4, 9}
    assert any(p["nblk"] > 256 for p in plans.values())
    assert all(p["waves"] == 4 for p in plans.values() if p["fwd_stream"])
    # the cases the table names for one path each
    want_stream = dict(smallest=1, one_tile=1, n37=0, phases=0, tail4=1, c7=1, many_images=1, l36=1, l37=0, ssd300_rows=0,
                       wide116=0, wide250=0, level3=1, level2=1, unnormalised=0, interleaved_ties=0, all_ties_1=0)
    for name, s in want_stream.items():
        assert plans[name]["fwd_stream"] == plans[name]["bwd_stream"] == s, (name, plans[name])
    for c, ot, op in lc.MISALIGNED:                      # a view 4, 8 or 12 bytes into a buffer: the tiled kernels' head and tail copies
        p = plans["%s+%d+%d" % (c.name, ot, op)]
        assert plans[c.name]["fwd_stream"] == 1 and p["fwd_stream"] == p["bwd_stream"] == 0, (c, ot, op)
    assert plans["l36"]["G"] == 9 and plans["l37"]["TA"] == plans["l36"]["TA"] == 128 and plans["phases"]["TA"] == 256
    assert plans["wide116"]["TA"] == plans["wide250"]["TA"] == 64
    # idle waves: fewer 64-anchor tiles in the whole batch than one workgroup has waves
    for name in ("smallest", "one_tile"):
        B, N, _ = next(c for c in lc.PATH if c.name == name).shape
        assert plans[name]["grid"] == 1 and B * ((N + 63) // 64) < plans[name]["waves"]
    # a last streaming tile of 4 anchors
    assert 68 % 64 == 4 and plans["tail4"]["fwd_stream"]
    assert plans["all_ties_1"]["nblk"] == 264 and plans["all_ties_1"]["gx"] == 64


def test_stream_switch_moves_every_case_to_the_tiled_kernels(lib, monkeypatch):
    monkeypatch.setenv("SSDHIP_LOSS_STREAM", "0")
    assert not any(p["fwd_stream"] or p["bwd_stream"] for p in _plans(lib).values())


@pytest.mark.parametrize("case", lc.LEVEL_CASES, ids=repr)
def test_no_knife_edges(case):
    """Any two distinct non-zero negative losses are at least 64 float32 steps apart: a condition (device logf is within a few ulp
    of NumPy's log), not a measurement."""
    _, parts = case.oracle()
    assert lc.min_step_gap(parts["neg_all"]) >= lc.MIN_STEPS


@pytest.mark.parametrize("case", lc.PATH + lc.WIDE, ids=repr)
def test_path_cases_select_something(case):
    loss, parts = case.oracle()
    assert parts["n_pos"] >= 1 and 0 < parts["k"] <= parts["n_neg_losses"]
    assert np.isfinite(loss).all() and (loss > 0).any()
    g = case.oracle_grad()
    assert np.isfinite(g).all() and (g[..., :-8] != 0).any()


@pytest.mark.parametrize("case", lc.ALL_TIES, ids=repr)
def test_all_ties_sweep_keeps_the_first_k(case):
    _, parts = case.oracle()
    K = case.kw["n_neg_min"]
    assert parts["k"] == K and parts["n_pos"] == 0
    assert np.array_equal(parts["keep"].reshape(-1) != 0, np.arange(lc.BIG_TOTAL) < K)
    assert np.unique(parts["neg_all"]).size == 1


def test_all_ties_sweep_covers_the_structural_boundaries():
    ks = set(lc.BIG_KS)
    assert {1, lc.ITEMS - 1, lc.ITEMS, lc.ITEMS + 1} <= ks                       # first / last of a thread's 8 values, first of the next thread
    assert {lc.CHUNK - 1, lc.CHUNK, lc.CHUNK + 1} <= ks                          # last of a pass block, first of the next
    assert {256 * lc.CHUNK - 1, 256 * lc.CHUNK, 256 * lc.CHUNK + 1} <= ks        # around the second round of the 256-block scan
    assert {lc.BIG_TOTAL - 1, lc.BIG_TOTAL} <= ks                                # the last tie left out / want == ties: no search


def test_interleaved_ties_cut_in_a_late_pass_block():
    c = lc.cut(lc.INTERLEAVED)
    _, parts = lc.INTERLEAVED.oracle()
    assert parts["k"] == lc.INTERLEAVED.kw["n_neg_min"]
    assert c["block"] >= 256 and 0 < c["kept"] == lc.INTERLEAVED_WANT < c["ties"]
    assert c["last"] + 1 != c["kept"]                                            # tie rank != flat index


def test_level3_case_shares_a_20_bit_prefix():
    _, parts = lc.LEVEL3.oracle()
    neg = parts["neg_all"].reshape(-1)
    levels = np.unique(neg[(neg > 1.0) & (neg < 2.0)])                           # -log(0.3002) = 1.2033; q = 0.01 gives 4.6
    assert levels.size == 12
    keys = lc.float_key(levels)
    assert np.unique(keys >> 12).size == 1 and np.unique(keys & 0xfff).size == 12
    c = lc.cut(lc.LEVEL3)
    assert c["thr"] in levels and 0 < c["kept"] < c["ties"]
    above = int((neg > c["thr"]).sum())
    assert int((neg > levels.max()).sum()) < above                               # want2 > 1: whole levels of the prefix lie above the cut


def test_level2_case_shares_the_top_key_byte():
    _, parts = lc.LEVEL2.oracle()
    neg = parts["neg_all"].reshape(-1)
    levels = np.unique(neg[(neg >= 0.5) & (neg < 2.0)])
    assert levels.size == 40
    keys = lc.float_key(levels)
    assert np.unique(keys >> 24).size == 1 and np.unique((keys >> 12) & 0xfff).size == 40
    c = lc.cut(lc.LEVEL2)
    assert c["thr"] in levels and 0 < c["kept"] < c["ties"]
    assert levels.min() < c["thr"] < levels.max()


def test_unnormalised_case_cuts_among_the_zeros():
    _, parts = lc.UNNORMALISED.oracle()
    neg = parts["neg_all"].reshape(-1)
    keep = parts["keep"].reshape(-1) != 0
    assert parts["k"] == parts["n_neg_losses"] == int((neg != 0).sum())
    assert (neg < 0).sum() > 1000 and not keep[neg < 0].any() and keep[neg > 0].all()
    c = lc.cut(lc.UNNORMALISED)
    assert c["thr"] == 0 and 0 < c["kept"] < c["ties"]
    zeros = np.flatnonzero(neg == 0)
    assert np.array_equal(np.flatnonzero(keep & (neg == 0)), zeros[:c["kept"]])   # the lowest flat indices, whatever the zero's sign
    pos = parts["positives"].reshape(-1) != 0
    assert (pos & keep).any() and (pos & ~keep).any() and (~pos & keep & (neg == 0)).any()
    assert pos[-5:].all() and np.signbit(neg[~pos & (neg == 0)]).all() and not np.signbit(neg[pos]).any()
