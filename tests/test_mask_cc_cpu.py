"""Hole and sprinkle removal (csrc/mask_cc.hip) without a GPU: the numpy / scipy reference the GPU tests compare with (tests/mask_cc_ref.py)
against answers worked out by hand, three wrong implementations it must tell apart, and the host side of the feature (constructor,
declarations, bindings, the tile constant)."""
import os
import re

import numpy as np

import mask_cc_ref as ref
from circuitvision_amd import _lib, sam2_infer
from circuitvision_amd.sam2_infer import SAM2Transforms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("cvmi_mask_cc_workspace", "cvmi_mask_components", "cvmi_mask_fill_small")


def planes(*rows_per_plane):
    """'#' = foreground (+1), '.' = background (-1) -> f32 [N, h, w]"""
    return np.stack([np.array([[1.0 if c == "#" else -1.0 for c in row] for row in rows], dtype=np.float32) for rows in rows_per_plane])


RING = planes(["......",
               ".###..",
               ".#.#..",
               ".###..",
               "......"])
HOLE_PAIR = planes(["#####",
                    "#.###",
                    "##.##",
                    "#####"])
SIZES = planes(["#########",
                "#.#..#..#",
                "#.#.##.##",
                "#########"])          # holes of area 1 + 1 = 2 (one column, 4-connected), 3 and 3


def test_diagonal_pair_is_one_component():
    x = planes(["#..",
                ".#.",
                "..."])
    lab, area, fg = ref.components(x, 0.0)
    assert lab[0].tolist() == [[1, 2, 2], [2, 1, 2], [2, 2, 2]]            # the background: one component, first pixel (0, 1) -> label 2
    assert area[0].tolist() == [[2, 7, 7], [7, 2, 7], [7, 7, 7]]
    assert fg[0].tolist() == [[True, False, False], [False, True, False], [False, False, False]]


def test_diagonal_background_pair_inside_foreground_is_one_hole():
    lab, area, _ = ref.components(HOLE_PAIR, 0.0)
    assert lab[0, 1, 1] == lab[0, 2, 2] == 1 + 1 * 5 + 1 and area[0, 1, 1] == area[0, 2, 2] == 2
    assert (lab[0][HOLE_PAIR[0] > 0] == 1).all() and (area[0][HOLE_PAIR[0] > 0] == 18).all()
    y = ref.fill_small(HOLE_PAIR, 0.0, 2, 0)
    assert y[0, 1, 1] == y[0, 2, 2] == 10.0 and np.array_equal(y[HOLE_PAIR > 0], HOLE_PAIR[HOLE_PAIR > 0])
    assert np.array_equal(ref.fill_small(HOLE_PAIR, 0.0, 1, 0), HOLE_PAIR)   # one hole of area 2, not two of area 1


def test_checkerboard_is_exactly_two_components():
    yy, xx = np.mgrid[0:7, 0:9]
    x = np.where((yy + xx) % 2 == 0, 1.0, -1.0).astype(np.float32)[None]
    lab, area, _ = ref.components(x, 0.0)
    assert sorted(np.unique(lab).tolist()) == [1, 2]
    assert (lab[0] == np.where((yy + xx) % 2 == 0, 1, 2)).all() and (area[0] == np.where((yy + xx) % 2 == 0, 32, 31)).all()


def test_ring_with_pinhole_becomes_a_filled_centre_and_a_deleted_ring():
    y = ref.fill_small(RING, 0.0, 8, 8)
    want = RING.copy()
    want[RING > 0] = -10.0                                                 # the ring: 8 pixels, a sprinkle
    want[0, 2, 2] = 10.0                                                   # the pinhole: area 1, judged on the ORIGINAL map
    assert np.array_equal(y, want)
    assert np.array_equal(ref.fill_small(RING, 0.0, 8, 7), np.where(want == -10.0, RING, want))     # ring of 8 survives a limit of 7
    assert np.array_equal(ref.fill_small(RING, 0.0, 0, 0), RING)


def test_area_equal_to_the_limit_is_filled_and_one_more_is_not():
    a = ref.components(SIZES, 0.0)[1][0]
    assert a[1, 1] == a[2, 1] == 2 and a[1, 3] == a[1, 4] == a[2, 3] == 3 and a[1, 6] == a[1, 7] == a[2, 6] == 3
    assert (ref.fill_small(SIZES, 0.0, 2, 0) == 10.0).sum() == 2
    assert (ref.fill_small(SIZES, 0.0, 3, 0) == 10.0).sum() == 8
    assert (ref.fill_small(SIZES, 0.0, 1, 0) == 10.0).sum() == 0


def test_fractional_limit():
    assert (ref.fill_small(SIZES, 0.0, 2.5, 0) == 10.0).sum() == 2          # areas 1 and 2, not 3
    assert (ref.fill_small(SIZES, 0.0, 0, 2.5) == -10.0).sum() == 0


def test_value_equal_to_the_threshold_is_background():
    x = np.full((1, 3, 3), 1.0, dtype=np.float32)
    x[0, 1, 1] = 0.37
    t = np.float32(0.37)
    x[0, 1, 1] = t
    lab, area, fg = ref.components(x, t)
    assert not fg[0, 1, 1] and area[0, 1, 1] == 1 and lab[0, 1, 1] == 5 and area[0, 0, 0] == 8
    y = ref.fill_small(x, t, 1, 0)
    assert y.dtype == np.float32 and y[0, 1, 1] == t + np.float32(10) and (y == 1.0).sum() == 8


def test_planes_stay_separate():
    x = planes(["...",
                "###"],
               ["###",
                "..."])
    lab, area, _ = ref.components(x, 0.0)
    assert lab[0, 1].tolist() == [4, 4, 4] and lab[1, 0].tolist() == [1, 1, 1] and (area == 3).all()
    y = ref.fill_small(x, 0.0, 0, 3)
    assert (y[x > 0] == -10.0).all()                                        # 3 + 3, never one component of 6


def _fill_sequential(x, t, hole, sprinkle):
    """WRONG: the sprinkles judged on the hole-filled map instead of the original"""
    y = ref.fill_small(x, t, hole, 0)
    return ref.fill_small(y, t, 0, sprinkle)


def _fill_strict(x, t, hole, sprinkle):
    """WRONG: `<` where the reference compares with `<=`"""
    _, areas, fg = ref.components(x, t)
    y = np.asarray(x, dtype=np.float32).copy()
    y[~fg & (areas < hole)] = np.float32(t) + np.float32(10)
    y[fg & (areas < sprinkle)] = np.float32(t) - np.float32(10)
    return y


def test_the_reference_tells_wrong_implementations_apart():
    # 4-connected labelling: the diagonal hole pair falls apart into two holes of area 1
    assert not np.array_equal(ref.fill_small(HOLE_PAIR, 0.0, 1, 0, structure=ref.FOUR), ref.fill_small(HOLE_PAIR, 0.0, 1, 0))
    assert not np.array_equal(ref.components(HOLE_PAIR, 0.0, structure=ref.FOUR)[0], ref.components(HOLE_PAIR, 0.0)[0])
    # sprinkles judged after the holes are filled: the ring has grown to 9 pixels and survives a limit of 8
    assert not np.array_equal(_fill_sequential(RING, 0.0, 8, 8), ref.fill_small(RING, 0.0, 8, 8))
    # `<`: an area equal to the limit stays
    assert not np.array_equal(_fill_strict(SIZES, 0.0, 3, 0), ref.fill_small(SIZES, 0.0, 3, 0))
    assert np.array_equal(_fill_strict(SIZES, 0.0, 4, 0), ref.fill_small(SIZES, 0.0, 3, 0))


def test_connected_components_contract():
    m = (RING[:, None] > 0)
    lab, cnt = ref.connected_components(m)
    assert lab.shape == cnt.shape == m.shape and lab.dtype == cnt.dtype == np.int32
    assert (lab[~m] == 0).all() and (cnt[~m] == 0).all() and (lab[m] == 1 + 6 + 1).all() and (cnt[m] == 8).all()
    assert np.array_equal(ref.connected_components(m.astype(np.uint8))[0], lab)


def test_transforms_keep_both_areas():
    tr = SAM2Transforms(256, 0.0, max_hole_area=8, max_sprinkle_area=8)
    assert tr.max_hole_area == 8 and tr.max_sprinkle_area == 8 and tr.fills_small_regions
    tr = SAM2Transforms(256, 0.0, max_hole_area=0.0, max_sprinkle_area=2.5)
    assert tr.max_hole_area == 0.0 and tr.max_sprinkle_area == 2.5 and tr.fills_small_regions
    tr = SAM2Transforms(256, 0.0)
    assert not tr.fills_small_regions
    marker = object()
    assert tr.fill_small_regions(marker) is marker                          # areas 0: the argument itself, nothing is touched


def test_entry_points_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "cvmi355.h")).read()
    for name in ENTRY_POINTS:
        decl = re.search(r"\b(?:int|size_t) %s\(([^;]*)\);" % name, header)
        assert decl, name
        assert name in _lib.SIGNATURES, name
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert int(re.search(r"#define CVMI_MASK_CC_TILE (\d+)", header).group(1)) == sam2_infer.MASK_CC_TILE
    assert callable(sam2_infer.get_connected_components)
