"""The encoder case table (tests/encode_cases.py) against the oracle alone, no GPU: every tie is a tie bit for bit, at the lane, wave
and tile distance its case names; every threshold case sits ON its threshold; the box-count ladder has the counts the launcher
branches on.  A case that loses what it is for fails here, not silently on the device.

Where the claims hold.  All of them hold for the three `coords` under border_pixels = 'half'.  Under 'include' and 'exclude' the box
areas carry d = +1 / -1 and only ties between anchors of EQUAL size survive (both sides go through the same operations on the same
numbers); ec.SIZE_BREAKS, all coords x {'include', 'exclude'}, is the `breaks` of the cases that compare anchors of different
size or need an IoU to equal a constant: row_tie_tiles, thresholds_equal, pos_equal, neg_equal.  pos_next_up and neg_next_up
("nothing but the bipartite matches") also hold under 'include', where the IoUs only get smaller, and break under 'exclude'
(ec.EXCLUDE_BREAKS), where they end up above the thresholds.  The test asserts both directions, so `breaks` is exact."""
import numpy as np
import pytest

from tests import encode_cases as ec

COMBOS = [(c, b) for c in ec.COORDS for b in ec.BORDERS]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _argmaxes(v):
    """Indices whose value equals the maximum of v bit for bit."""
    return tuple(int(i) for i in np.nonzero(_bits(v) == _bits(v.max()))[0])


def _distance(cols, distance):
    if distance == "lane":
        return cols[0] // 64 == cols[1] // 64 and cols[0] != cols[1]
    if distance == "wave":
        return any(a // 64 != b // 64 and a // 256 == b // 256 for a in cols for b in cols)
    assert distance == "tile"
    return any(a // 256 != b // 256 for a in cols for b in cols)


def _bipartite(case, image, **over):
    from oracle import np_oracle as orc
    return orc.match_bipartite_greedy(ec.similarities(case, image, **over))


def claim_holds(case, claim, coords, border):
    over = dict(coords=coords, border_pixels=border)
    kind, image = claim[0], claim[1]
    sim = ec.similarities(case, image, **over)
    kw = case.config(**over)
    if kind == "row":
        _, _, row, cols, distance = claim
        return _argmaxes(sim[row]) == tuple(cols) and len(cols) >= 2 and _distance(cols, distance)
    if kind == "rows":
        _, _, (r, s), same = claim
        return r < s and _bits(sim[r].max()) == _bits(sim[s].max()) and sim[r].max() > 0 and (int(np.argmax(sim[r])) == int(np.argmax(sim[s]))) == same
    if kind == "rescan":
        _, _, row, taken, cols, distance = claim
        v = sim[row].copy()
        v[list(taken)] = 0
        return _argmaxes(v) == tuple(cols) and v.max() > 0 and (len(cols) == 1 or _distance(cols, distance))
    if kind == "column":
        _, _, anchor, rows = claim
        return (_argmaxes(sim[:, anchor]) == tuple(rows) and len(rows) >= 2 and anchor not in _bipartite(case, image, **over)
                and sim[rows[0], anchor] >= kw["pos_iou_threshold"])
    if kind == "claimed":
        _, _, anchor, rows = claim
        return all(int(_bipartite(case, image, **over)[r]) == anchor for r in rows)
    if kind == "zero_row":
        return not sim[claim[2]].any()
    if kind in ("on_pos", "on_neg"):
        _, _, row, cols = claim
        thr = kw["pos_iou_threshold" if kind == "on_pos" else "neg_iou_limit"]
        return bool(np.all(_bits(sim[row, list(cols)]) == _bits(thr))) and _argmaxes(sim[row]) == tuple(cols)
    assert kind == "only_bipartite"
    mm = case.oracle(**over)[1][image]
    g = case.gt[image].shape[0]
    return int((mm >= 0).sum()) == g and not (mm == -2).any()


@pytest.mark.parametrize("case", ec.TIES + ec.QUIRKS + ec.THRESHOLDS, ids=repr)
def test_claims_hold_where_the_case_says(case):
    assert case.claims
    for coords, border in COMBOS:
        held = [claim_holds(case, claim, coords, border) for claim in case.claims]
        if case.holds(coords, border):
            assert all(held), (case, coords, border, [c for c, h in zip(case.claims, held) if not h])
        else:
            assert not all(held), "%s: listed as broken under %s / %s, but every claim holds" % (case, coords, border)
    for coords in ("corners", "centroids"):                # the two the issue requires of every tie case
        assert case.holds(coords, "half")


def test_anchor_layout_is_the_documented_one():
    from oracle import np_oracle as orc
    a = orc.EncoderOracle(**ec.DYADIC).anchors()
    assert a.shape == (ec.N_ANCHORS, 4)
    n = lambda i, j: 16 * i + j
    assert a[n(6, 2)].tolist() == [12, 44, 28, 60] and a[256 + 8 * 1 + 1].tolist() == [8, 8, 40, 40] and a[320 + 4 * 1 + 2].tolist() == [48, 16, 112, 80]
    assert np.all(a == np.round(a)) and np.all(a % 4 == 0)
    assert orc.EncoderOracle(**ec.ODD_N).anchors().shape == (ec.N_ANCHORS_ODD, 4)


def test_issue_values_on_the_oracle():
    """The numbers quoted in the issue, corners / half."""
    from oracle import np_oracle as orc
    a = orc.EncoderOracle(**ec.DYADIC).anchors()
    for box, value, cols in ((ec.TILES, 0.5, (34, 35, 265)), (ec.LANES, 0.6, (97, 98)), (ec.FULL, 0.25, (325, 326, 329, 330))):
        row = orc.iou(np.array([box]), a, coords="corners", mode="outer_product", border_pixels="half")[0]
        assert _argmaxes(row) == cols and row.max() == value


def test_threshold_steps_are_single_steps():
    up = {c.name: c for c in ec.THRESHOLDS}
    assert up["pos_next_up"].config()["pos_iou_threshold"] == np.nextafter(0.5, 1) > 0.5
    assert up["neg_next_up"].config()["neg_iou_limit"] == np.nextafter(0.25, 1) > 0.25
    # on the threshold the anchors ARE matched / neutral, one step up they are not
    assert (up["pos_equal"].oracle()[1][0, [34, 35, 265]] == 0).all() and (up["pos_next_up"].oracle()[1][0, [35, 265]] == -1).all()
    assert up["neg_equal"].oracle()[1][0, [325, 326, 329, 330]].tolist() == [0, -2, -2, -2]
    assert up["neg_next_up"].oracle()[1][0, [325, 326, 329, 330]].tolist() == [0, -1, -1, -1]
    both = up["thresholds_equal"].oracle()[1][0]
    assert both[[34, 35, 265]].tolist() == [0, 0, 0] and both[[325, 326, 329, 330]].tolist() == [2, -2, -2, -2]


def test_outcomes_the_cases_are_for():
    """What the device must reproduce, spelled out once on the oracle (multi, corners, half)."""
    by = {c.name: c for c in ec.NAMED}
    mm = lambda name, image=0, **over: by[name].oracle(**over)[1][image]
    assert mm("row_tie_lanes")[[97, 98]].tolist() == [0, 0] and mm("row_tie_lanes", matching_type="bipartite")[[97, 98]].tolist() == [0, -2]
    assert mm("row_tie_waves", matching_type="bipartite")[[53, 69]].tolist() == [0, -2]
    assert mm("row_tie_tiles", matching_type="bipartite")[[34, 35, 265]].tolist() == [0, -2, -2]
    assert mm("duplicate_boxes", matching_type="bipartite")[[97, 98]].tolist() == [0, 1]       # the third copy takes what is left of its row
    assert mm("rescan_tie_waves", matching_type="bipartite")[[53, 54, 69, 70]].tolist() == [0, 1, -2, -2]
    assert mm("multi_tie_two_boxes")[[82, 97, 98]].tolist() == [0, 1, 0]
    assert mm("column_claimed_twice")[0] == 1 and mm("zero_row_first")[[0, 53]].tolist() == [2, 1]
    assert mm("zero_row_last")[[0, 53, 97]].tolist() == [2, 0, 1]           # 53 is matched again, by the multi match; bipartite alone:
    assert mm("zero_row_last", matching_type="bipartite")[[0, 53, 97]].tolist() == [2, -2, 1]
    big = by["more_boxes_than_anchors"]
    assert [g.shape[0] for g in big.gt] == [0, ec.N_ANCHORS + 4, 1]
    assert len(set(map(tuple, big.gt[1][:, 1:]))) > ec.N_ANCHORS           # more DIFFERENT boxes than anchors


def test_ladder_counts_and_the_48k_step():
    assert ec.GTBOX_BYTES == 4 * 8 + 5 * 8 + 8                             # lab[4], PxBox {x0, y0, x1, y1, area}, cls + padding
    assert ec.match_lds_bytes(ec.G48 - 1) <= 48 * 1024 < ec.match_lds_bytes(ec.G48) and ec.G48 == 491
    assert ec.LADDER == (1, 63, 64, 65, 256, 257, 490, 491, 1024)
    assert ec.match_lds_bytes(ec.ENC_MAX_GT) <= 150 * 1024                  # the launcher's own ceiling is never the reason
    for count in ec.LADDER:
        gt = ec.ladder(count).gt
        assert [g.shape[0] for g in gt] == [0, count, 1]
        boxes, copies = np.unique(gt[1][:, 1:], axis=0, return_counts=True)
        assert copies.max() == (8 if count >= 16 else 1)
        w, h = gt[1][:, 3] - gt[1][:, 1], gt[1][:, 4] - gt[1][:, 2]
        assert w.min() >= 4 and h.min() >= 4 and w.max() <= 28 and h.max() <= 28


def test_class_counts_select_every_tile_size():
    assert {C: (C + 12, ec.finalize_tile(C + 12, 4), ec.finalize_tile(C + 12, 8)) for C in ec.CLASS_TABLE} == ec.CLASS_TABLE
    assert {v[1] for v in ec.CLASS_TABLE.values()} == {v[2] for v in ec.CLASS_TABLE.values()} == {256, 128, 64}
    for case in ec.CLASSES:
        C = case.config()["n_classes"] + 1
        assert len(case.gt) == 3 and max(g[:, 0].max() for g in case.gt if g.size) == C - 1
        y, mm = case.oracle()
        assert y.shape == (3, ec.N_ANCHORS, C + 12) and (mm >= 0).any() and (mm == -2).any() and (mm[1] == -1).all()
    # N = 336 and every tile start are multiples of 4: a float32 tile's phase is its buffer's alone; N = 329 moves it per image
    assert ec.N_ANCHORS % 4 == 0 and {(b * ec.N_ANCHORS_ODD * 17) % 4 for b in range(3)} == {0, 1, 2}
