"""The power of the detector-tail matrix, proven without a GPU (tests/detect_ref.py, op_matrix.NMS_ROWS / DECODE_ROWS): the fp64 decode is the
decode, its bound is what the fp32 statement needs, every NMS row holds exactly the candidates it claims, the numpy restatement equals the
oracle, and a reference that makes one of the classic mistakes of these kernels changes the expected output of the rows meant to catch it."""
import numpy as np
import pytest
import torch

import detect_ref as R
from op_matrix import (DECODE_ROWS, DETECT_MUTANT_ROWS, DETECT_UNSEEN_MUTANTS, NMS_MAX_NMS, NMS_ROWS, decode_seams, nms_pick)

NMS_BY_ID = {r["id"]: r for r in NMS_ROWS}
DEC_BY_ID = {r["id"]: r for r in DECODE_ROWS}


# ---- decode ------------------------------------------------------------------------------------------------------------------------------------
def test_the_decode_bound_is_the_measured_deviation_of_the_fp32_statement():
    dev = R.measure_dec_dev()
    assert set(dev) == set(R.DEC_DEV) and R.FACTOR == 4.0
    for key, ms in sorted(dev.items()):
        for m, c in zip(ms, R.DEC_DEV[key]):
            print(f"{key}: measured {m:.4e}  constant {c:.4e}")
            assert m <= c, f"{key}: measured {m!r} is past detect_ref.DEC_DEV: the rows changed, update the constant"
            assert c <= 4 * m, f"{key}: detect_ref.DEC_DEV is more than 4 x the measured {m!r}: tighten it"


def test_the_decode_bound_stays_below_half_of_the_hand_set_tolerances_where_they_scale():
    """test_yolo_gpu.test_detect_decode allows 2e-3 (1 + |ref|) in fp16 and 1e-5 (1 + |ref|) in f32.  Class rows stay far below half of either.  Box
    rows do in fp16; in f32 they do from |ref| = 0.6 S on, and exceed it where a centre or size cancels to a small value: the fp32 statement itself
    is off by 1.5e-7 S there (7e-5 at S = 496), which 1e-5 never covered -- that test compares two fp32 computations with each other, not with fp64."""
    for row in DECODE_ROWS:
        for dt in row["dtypes"]:
            _, _, ref = R.decode_case(row["id"], dt)
            hand = (2e-3 if dt == "f16" else 1e-5) * (1 + ref.abs())
            assert bool((R.dec_bound(ref[:, 4:], "cls", dt) <= hand[:, 4:] / 2).all()), (row["id"], dt)
            box = R.dec_bound(ref[:, :4], "box", dt, row)
            if dt == "f16":
                assert bool((box <= hand[:, :4] / 2).all()), row["id"]
            else:
                S = R.decode_scale(row).expand_as(ref[:, :4])
                assert bool((box <= hand[:, :4] / 2)[ref[:, :4].abs() >= 0.6 * S].all()), row["id"]


def test_the_fp64_decode_gives_the_by_hand_answer():
    """One anchor at (0, 0), stride 8: left = 3, top = the mean of bins 0 and 2, right = 5, bottom = 2; class logits 0 and ln 3."""
    box = torch.full((1, 1, 1, 64), -1000.0)
    box[0, 0, 0, 3] = 0.0
    box[0, 0, 0, 16 + 0] = box[0, 0, 0, 16 + 2] = 7.0
    box[0, 0, 0, 32 + 5] = -2.0
    box[0, 0, 0, 48 + 2] = 11.0
    cls = torch.tensor([0.0, float(np.log(3.0))], dtype=torch.float64).view(1, 1, 1, 2)
    out = R.decode_ref([(box, cls)])
    x1, y1, x2, y2 = 0.5 - 3, 0.5 - 1, 0.5 + 5, 0.5 + 2
    want = torch.tensor([(x1 + x2) / 2 * 8, (y1 + y2) / 2 * 8, (x2 - x1) * 8, (y2 - y1) * 8, 0.5, 0.75], dtype=torch.float64)
    assert out.shape == (1, 6, 1) and float((out[0, :, 0] - want).abs().max()) < 1e-12, out
    assert R.best_ref(out[:, 4:])[1].tolist() == [[1]]


def test_best_class_excuses_stay_under_one_percent_and_tie_rows_have_ties():
    for row in DECODE_ROWS:
        for dt in row["dtypes"]:
            _, levels, ref = R.decode_case(row["id"], dt)
            if row["kind"] == "rand":
                frac = float(R.excused_anchors(ref, dt).float().mean())
                print(f"{row['id']} {dt}: {frac:.4f} of the anchors excused from the reference's argmax")
                assert frac <= 0.01, (row["id"], dt, frac)
            else:                                                              # excused from nothing: the class comes from the logits alone
                exact = R.decode_exact_cls(row, levels)
                top = ref[:, 4:].topk(2, dim=1).values
                tied = (top[:, 0] - top[:, 1]) <= R.dec_bound(top[:, 0], "cls", dt)
                assert float(tied.float().mean()) > 0.25, (row["id"], "the row is there for its ties")
                first, last = R.best_ref(ref[:, 4:])[1], R.best_ref(ref[:, 4:], "best_last_max")[1]
                assert bool(((exact == first) | tied).all()) and bool((exact <= last).all()), row["id"]


def test_decode_rows_state_their_seams():
    for row in DECODE_ROWS:
        seams = decode_seams(row)
        for kind in ("image", "level1", "level2"):
            inside = [g for g in seams[kind] if g % 64 != 0]
            if kind in row["straddle"]:
                assert inside, f"{row['id']}: no {kind} seam falls inside a 64-anchor workgroup"
        assert len(row["levels"]) >= 2 or not seams["level1"]
    total = {r["id"]: r["B"] * r["A"] for r in DECODE_ROWS}
    assert total["l1_64"] == 64 and total["l1_1"] == 1 and total["l3_seams"] % 64 != 0
    assert {len(r["levels"]) for r in DECODE_ROWS} == {1, 2, 3}
    assert any((1, 1) in r["levels"] and len(r["levels"]) == 3 for r in DECODE_ROWS) and any(h != w for r in DECODE_ROWS for h, w in r["levels"])
    for want in ("image", "level1", "level2"):
        assert any(want in r["straddle"] for r in DECODE_ROWS), want


# ---- NMS ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rid", [r["id"] for r in NMS_ROWS])
def test_every_nms_row_holds_its_candidates_and_the_restatement_equals_the_oracle(rid):
    row, pred, det, idx = R.nms_case(rid)
    conf = np.float32(row["conf"])
    best = pred[:, 4:].max(1).values.numpy()
    assert ((best > conf).sum(1) == row["n"]).all()
    if row["n"] < row["A"]:
        assert ((best == conf).sum(1) >= 1).all(), "some anchors sit at exactly conf_thres"
    assert (row["gk"], row["P"], row["Ps"], row["nthr"], row["geo_lds"]) == nms_pick(row["A"], row["n"])
    assert R.same_detections((det, idx), R.nms_variant(pred, row["conf"], row["iou"], row["max_det"], row["max_wh"])), rid
    counts = [d.shape[0] for d in det]
    if row["survivors"]:
        free = R.nms_variant(pred, row["conf"], row["iou"], 1 << 30, row["max_wh"])[0]
        assert all(eval("%d %s" % (d.shape[0], row["survivors"])) for d in free), (rid, [d.shape[0] for d in free])
        assert all(c == min(row["max_det"], d.shape[0]) for c, d in zip(counts, free))
    if row["iou"] >= 0 and row["kind"] != "maxnms" and row["n"] > 3:
        assert all(min(2, row["max_det"]) <= c for c in counts) and (row["kind"] == "isolated" or all(c < row["n"] for c in counts)), (rid, counts, "something is kept, something suppressed")
    if row["iou"] < 0:
        assert not bool((pred[:, 2:4] == 0).any()) and counts == [1] * row["B"]


def test_the_degenerate_rows_are_what_they_claim():
    _, pred, det, idx = R.nms_case("zero_area")
    wh = pred[:, 2:4]
    assert bool(((wh[:, 0] == 0) & (wh[:, 1] == 0)).any()) and bool(((wh[:, 0] == 0) & (wh[:, 1] > 0)).any())
    assert any(bool(((d[:, 2] - d[:, 0]) * (d[:, 3] - d[:, 1]) == 0).sum() > 10) for d in det), "duplicated zero-area boxes all survive"
    _, pred, det, _ = R.nms_case("dups")
    assert len(torch.unique(pred[0, :4].T, dim=0)) <= 12
    _, pred, det, idx = R.nms_case("ties")
    assert all(len(torch.unique(d[:, 4])) == 1 and bool((i[1:] > i[:-1]).all()) for d, i in zip(det, idx)), "one score: kept in anchor order"
    _, pred, det, _ = R.nms_case("clsoff")
    for d in det:                                                          # every cell keeps its box once per class
        boxes, inv = torch.unique(d[:, :4], dim=0, return_inverse=True)
        per_cell = [sorted(d[inv == k, 5].tolist()) for k in range(len(boxes))]
        assert all(len(set(c)) == len(c) for c in per_cell) and sum(c == [0.0, 60.0, 61.0] for c in per_cell) >= 20
    _, pred, det, _ = R.nms_case("iou0_touch")
    assert all(d.shape[0] > pred.shape[2] // 3 for d in det), "touching boxes survive at iou_thres = 0"


def test_the_rounding_row_holds_pairs_whose_verdict_hangs_on_fp32_rounding():
    cell, bi, bj, v32 = R.offset_flips()
    print(f"class-offset search: {len(cell)} of {R.ROUNDING_SEARCH} seeded pairs flip;  contraction search: {len(R.fma_flips()[0])}")
    assert len(cell) == R.ROUNDING_FOUND["offset"] and len(R.fma_flips()[0]) == R.ROUNDING_FOUND["fma"]
    pairs = R.rounding_pairs()
    assert sum(c == R.ROUNDING_CLASS for c, *_ in pairs) >= 20 and sum(c == 0 for c, *_ in pairs) >= 20
    row, pred, det, idx = R.nms_case("rounding")
    kept = {tuple(r) for r in det[0][:, :4].tolist()}
    thr = np.float32(row["iou"])
    for c, b1, b2, verdict in pairs:                                          # the oracle's own arithmetic gives the searched verdict
        x1, x2 = R._xyxy32(b1[None])[0], R._xyxy32(b2[None])[0]
        assert tuple(x1.tolist()) in kept and (tuple(x2.tolist()) in kept) == (not verdict)
        off = np.full(1, np.float32(c) * np.float32(row["max_wh"]))
        plain = bool(R.iou32(x1[None], x2[None], off)[0] > thr)
        assert plain == verdict
        if c == R.ROUNDING_CLASS:
            assert plain != bool(R._iou64(x1[None], x2[None])[0] > float(thr))
        else:
            assert plain != bool(R.iou32(x1[None], x2[None], off, fma=True)[0] > thr)


def test_max_nms_row_counts():
    row, pred, det, idx = R.nms_case("max_nms")
    free = R.nms_variant(pred, row["conf"], row["iou"], row["max_det"], row["max_wh"], mutant="no_max_nms")
    assert row["n"] > NMS_MAX_NMS and [d.shape[0] for d in det] == [40] and [d.shape[0] for d in free[0]] == [140]


# ---- mutants -----------------------------------------------------------------------------------------------------------------------------------
def _decode_mutant_seen(row, dt, mutant):
    _, levels, ref = R.decode_case(row["id"], dt)
    if mutant == "best_last_max":
        return not torch.equal(R.best_ref(ref[:, 4:])[1], R.best_ref(ref[:, 4:], mutant)[1]) and \
            not torch.equal(R.decode_exact_cls(row, levels), R.best_ref(ref[:, 4:], mutant)[1])
    m = R.decode_ref(levels, mutant=mutant)
    if not bool(torch.isfinite(m).all()):
        return True
    return R.dec_ratio(m[:, :4], ref[:, :4], "box", dt, row)[0] > 1.0 or R.dec_ratio(m[:, 4:], ref[:, 4:], "cls", dt)[0] > 1.0


def _mutant_seen(mutant, rid):
    if rid.endswith(":decode"):
        row = DEC_BY_ID[rid[:-7]]
        return all(_decode_mutant_seen(row, dt, mutant) for dt in row["dtypes"])
    row, pred, det, idx = R.nms_case(rid)
    return not R.same_detections((det, idx), R.nms_variant(pred, row["conf"], row["iou"], row["max_det"], row["max_wh"], mutant=mutant))


@pytest.mark.parametrize("mutant,rid", [(m, rid) for m, rids in DETECT_MUTANT_ROWS.items() for rid in rids])
def test_each_mutant_changes_the_expected_output_of_its_rows(mutant, rid):
    assert _mutant_seen(mutant, rid), f"{mutant} passes on {rid}: change the row, never the comparison"


def test_every_mutant_has_rows_or_is_listed_as_unseen():
    names = set(R.NMS_MUTANTS) | set(R.DECODE_MUTANTS)
    assert set(DETECT_MUTANT_ROWS) | set(DETECT_UNSEEN_MUTANTS) == names and not set(DETECT_MUTANT_ROWS) & set(DETECT_UNSEEN_MUTANTS)
    ids = set(NMS_BY_ID) | {r + ":decode" for r in DEC_BY_ID}
    assert all(rids and set(rids) <= ids for rids in list(DETECT_MUTANT_ROWS.values()) + list(DETECT_UNSEEN_MUTANTS.values()))
    for mutant, rids in DETECT_UNSEEN_MUTANTS.items():                          # a recorded blind spot stays blind (or moves to DETECT_MUTANT_ROWS)
        assert not any(_mutant_seen(mutant, rid) for rid in rids), mutant
    assert any(r.endswith(":decode") for r in DETECT_MUTANT_ROWS["best_last_max"]) and any(not r.endswith(":decode") for r in DETECT_MUTANT_ROWS["best_last_max"])
