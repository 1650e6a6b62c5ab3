"""The automatic mask generator's reference (tests/amg_ref.py) against known answers written by hand, the proof that every deliberately wrong
variant (AMG_MUTANTS) changes at least one of them, the preconditions of the scorer's GPU rows (every pixel of the fp64 reference clear of every
level), and the C ABI's bookkeeping.  No GPU, no library."""
import math
import os
import re

import numpy as np
import pytest
import torch

import amg_ref as ref
from amg_ref import AMG_MUTANTS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "circuitvision_amd", "csrc")

# a 4 x 4 map whose three counts differ: levels -1 / 0 / 1
MAP4 = torch.tensor([[-2.0, -1.0, -0.5, 0.0],
                     [0.5, 1.0, 2.0, 3.0],
                     [-3.0, -0.25, 0.25, 1.5],
                     [-1.5, -2.5, 0.75, -0.75]])
# an L: column 1 rows 0..3 and row 3 columns 1..3
L_MAP = torch.full((5, 6), -4.0)
L_MAP[0:4, 1] = 4.0
L_MAP[3, 1:4] = 4.0


def _case_counts(mutant=None):
    return ref.score_planes(MAP4[None], -1.0, 0.0, 1.0, mutant)[0].tolist()


def _case_boundary(mutant=None):
    """Values exactly ON each level: a strict comparison counts none of them."""
    m = torch.tensor([[-1.0, 0.0, 1.0, -5.0]])
    return ref.score_planes(m[None], -1.0, 0.0, 1.0, mutant)[0].tolist()


def _case_boxes(mutant=None):
    maps = torch.stack([L_MAP, torch.full((5, 6), -4.0)])
    return ref.score_planes(maps, -1.0, 0.0, 1.0, mutant)[:, 3:7].tolist()


def _case_nms_order(mutant=None):
    """Equal scores: the lower index first; a better score further down the list comes before both."""
    boxes = [[0, 0, 10, 10], [20, 20, 30, 30], [40, 40, 50, 50]]
    return ref.nms(boxes, [0.9, 0.9, 0.95], 0.5, mutant).tolist()


def _case_generate(mutant=None):
    """Two points x one candidate + one padding point whose plane would pass; maps 4 x 6."""
    a = torch.full((4, 6), -4.0)
    a[1:3, 1:4] = 4.0
    b = torch.full((4, 6), -4.0)
    b[0:2, 3:6] = 4.0
    pad = torch.full((4, 6), -4.0)
    pad[3, 0:2] = 4.0
    maps = torch.stack([a, b, pad])
    out = ref.generate_ref(None, np.array([[0.9], [0.95], [0.99]], dtype=np.float32), maps, ref.point_grid(2), 2, 4, 6, 0.5, 0.9, ref.levels(0.0, 1.0), 0.7, mutant)
    return [(d["area"], d["bbox"], d["predicted_iou"], d["point_coords"], d["stability_score"], d["segmentation"].tolist()) for d in out]


CASES = (_case_counts, _case_boundary, _case_boxes, _case_nms_order, _case_generate)


def test_point_grid_2():
    assert ref.point_grid(2).tolist() == [[0.25, 0.25], [0.75, 0.25], [0.25, 0.75], [0.75, 0.75]]
    g = ref.point_grid(32)
    assert g.shape == (1024, 2) and g[0].tolist() == [1 / 64, 1 / 64] and g[1, 1] == g[0, 1] and g[1, 0] > g[0, 0]       # x fastest
    from circuitvision_amd.amg import build_point_grid
    assert np.array_equal(build_point_grid(32), g) and np.array_equal(build_point_grid(3), ref.point_grid(3))


def test_three_counts_of_a_4x4_map():
    # > 1: 2, 3, 1.5 -> 3;  > -1: everything but -2, -1, -3, -1.5, -2.5 -> 11;  > 0: 0.5, 1, 2, 3, 0.25, 1.5, 0.75 -> 7
    assert _case_counts() == [3, 11, 7, 0, 1, 3, 3, 0]
    assert _case_boundary() == [0, 2, 1, 2, 0, 2, 0, 0]                  # -1, 0, 1, -5 against -1 / 0 / 1: on a level is not above it
    assert float(ref.stability(np.array([[3, 11, 7, 0, 0, 0, 0, 0]]))[0]) == float(np.float32(3) / np.float32(11))
    assert math.isnan(float(ref.stability(np.array([[0, 0, 0, 0, 0, 0, 0, 0]]))[0]))


def test_levels_are_rounded_once_from_double():
    assert ref.levels(0.0, 1.0) == (-1.0, 0.0, 1.0) and ref.levels(0.5, 0.0) == (0.5, 0.5, 0.5)
    lo, mid, hi = ref.levels(0.1, 0.3)
    assert lo == float(np.float32(0.1 - 0.3)) and hi == float(np.float32(0.1 + 0.3)) and mid == float(np.float32(0.1))
    assert lo != float(np.float32(0.1) - np.float32(0.3))               # not the difference of the rounded values


def test_box_of_an_L_and_of_the_empty_mask():
    assert _case_boxes() == [[1, 0, 3, 3], [0, 0, 0, 0]]


def test_iou_exactly_at_the_threshold_keeps_both():
    # [0,0,10,10] and [0,0,10,5] (areas 100 and 50, intersection 50): IoU = 50 / 100 = 0.5 exactly; suppression needs IoU > threshold
    assert ref.nms([[0, 0, 10, 10], [0, 0, 10, 5]], [0.9, 0.8], 0.5).tolist() == [0, 1]
    assert ref.nms([[0, 0, 10, 10], [0, 0, 10, 6]], [0.9, 0.8], 0.5).tolist() == [0]


def test_equal_scores_keep_the_lower_index_first():
    assert _case_nms_order() == [2, 0, 1]
    assert ref.nms([[0, 0, 10, 10], [0, 0, 10, 10]], [0.7, 0.7], 0.5).tolist() == [0]


def test_one_pixel_mask_is_kept():
    """A one-pixel mask's box has area 0: against itself-like boxes the IoU is 0 / 0 = NaN, which does not suppress."""
    assert ref.nms([[3, 3, 3, 3], [3, 3, 3, 3], [0, 0, 8, 8]], [0.9, 0.8, 0.7], 0.1).tolist() == [0, 1, 2]


def test_select_drops_nan_stability_equal_iou_and_padding():
    stats = np.array([[9, 10, 9, 0, 0, 1, 1, 0], [0, 0, 0, 0, 0, 0, 0, 0], [10, 10, 10, 0, 0, 1, 1, 0], [10, 10, 10, 0, 0, 1, 1, 0], [10, 10, 10, 0, 0, 1, 1, 0]])
    iou = np.array([0.9, 0.9, 0.5, 0.9, 0.9], dtype=np.float32)
    assert ref.select(stats, iou, 4, 0.5, 0.9).tolist() == [0, 3]       # 1: NaN stability; 2: iou == threshold; 4: padding
    assert ref.select(stats, iou, 4, 0.5, 0.9, "padding_selected").tolist() == [0, 3, 4]
    assert ref.select(stats, iou, 4, 0.5, 0.95).tolist() == [3]         # 9 / 10 < 0.95


def test_generate_ref_known_answer():
    out = _case_generate()
    # candidate 1 (iou 0.95) first, then candidate 0; the padding plane (iou 0.99) is never selected
    assert [o[2] for o in out] == [float(np.float32(0.95)), float(np.float32(0.9))]
    assert out[0][:2] == (6, [3, 0, 2, 1]) and out[1][:2] == (6, [1, 1, 2, 1])
    assert out[0][3] == [[0.75 * 6, 0.25 * 4]] and out[1][3] == [[0.25 * 6, 0.25 * 4]]
    assert out[0][4] == 1.0


@pytest.mark.parametrize("mutant", AMG_MUTANTS)
def test_every_mutant_changes_a_case(mutant):
    changed = [c.__name__ for c in CASES if c(mutant) != c()]
    assert changed, mutant


def _amg_constants():
    text = open(os.path.join(CSRC, "mask_amg.hip")).read()
    cap = int(re.search(r"constexpr int AMG_GRID_CAP = (\d+);", text).group(1))
    threads = int(re.search(r"constexpr int AMG_THREADS = (\d+);", text).group(1))
    cols = int(re.search(r"constexpr int AMG_COLS = (\d+);", text).group(1))
    assert "constexpr int AMG_CHUNK = AMG_THREADS * AMG_COLS;" in text
    return cap, threads * cols


def scorer_rows():
    return ref.SCORER_ROWS + (ref.grid_cap_row(*_amg_constants()),)


@pytest.mark.parametrize("row", scorer_rows(), ids=lambda r: r[0])
def test_scorer_rows_are_clear_of_every_level_on_every_pixel(row):
    assert ref.scorer_clear(row), row[0]
    M, H, W = row[1], row[4], row[5]
    assert tuple(ref.scorer_reference(row).shape) == (M, H, W)


def test_scorer_rows_cover_what_they_claim():
    rows = {r[0]: r for r in scorer_rows()}
    cap, chunk = _amg_constants()
    assert rows["grid_cap_plus_1"][4] * rows["grid_cap_plus_1"][5] == cap * chunk + 1
    flat = ref.score_planes(ref.scorer_reference(rows["flat"]), -1.0, 0.0, 1.0)
    assert flat[0].tolist() == [0, 0, 0, 0, 0, 0, 0, 0] and flat[1].tolist() == [143, 143, 143, 0, 0, 10, 12, 0]       # all below, all above
    edge = ref.score_planes(ref.scorer_reference(rows["edge"]), -1.0, 0.0, 1.0)
    H, W = rows["edge"][4], rows["edge"][5]
    assert all(e[3] == 0 and e[4] == 0 and e[5] == W - 1 and e[6] == H - 1 for e in edge.tolist())                   # the blob touches all four borders
    exact = rows["exact_4x"]
    assert (exact[4], exact[5]) == (4 * exact[2], 4 * exact[3])
    s = ref.score_planes(ref.scorer_reference(rows["up_67x131"]), -1.0, 0.0, 1.0)
    assert all(r[0] < r[2] < r[1] for r in s.tolist())                   # the three counts differ on every plane


def test_entry_points_are_declared_and_bound():
    from circuitvision_amd import _lib
    header = open(os.path.join(ROOT, "include", "cvmi355.h")).read()
    for name in ("cvmi_amg_score", "cvmi_amg_select"):
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    fields = re.search(r"typedef struct cvmi_amg_record \{(.*?)\} cvmi_amg_record;", header, re.S).group(1)
    names = [n.strip() for part in re.findall(r"^\s*(?:float|int) ([^;]*);", fields, re.M) for n in part.split(",")]
    assert names == [n for n, _ in _lib.AMG_RECORD] and np.dtype(_lib.AMG_RECORD).itemsize == 4 * len(names)
    text = open(os.path.join(CSRC, "mask_amg.hip")).read()
    assert "CVMI_ENTRY" not in text and "getenv" not in text
    assert '#include "bilinear.hpp"' in text and all('#include "bilinear.hpp"' in open(os.path.join(CSRC, f)).read() for f in ("resample.hip", "sam_ops.hip"))
    assert "mask_amg.o" in open(os.path.join(CSRC, "Makefile")).read()
