"""The geometric contour oracle (tests/contour_ref.py) is validated here before it judges a kernel: tests/wire_ref.py's trace satisfies every
rule on every row of op_matrix.CONTOUR_ROWS (so no row asks the GPU for what the reference cannot give), hand-stated answers hold, each
mutant of a correct answer is rejected under the name of the rule it breaks, and the one-channel fixed-point resize cvmi_node_prepare is
compared with is measured against a float64 bilinear resize."""
import functools

import numpy as np
import pytest

import wire_ref as W
from contour_ref import (RULES, build_plane, check_plane, external_components, foreground, plane_inverts, prepare_boxes, prepare_plane, resize_bilinear_f64,
                         shoelace2)
from op_matrix import CONTOUR_CAPACITY_ROW, CONTOUR_ROWS, PREPARE_HEIGHT, PREPARE_REFUSED, PREPARE_ROWS, plane_shape
from oracle.preprocess import resize_linear_u8

ALL_ROWS = CONTOUR_ROWS + [CONTOUR_CAPACITY_ROW]


@functools.lru_cache(maxsize=None)
def wire_ref_contours(spec, sums):
    """((points, 2 x signed area, rect), ...) of one plane spec from tests/wire_ref.py, the bit-for-bit reference of the GPU test; shared by
    every row that holds the plane."""
    plane = build_plane(spec)
    p = 255 - plane if (sums and W.plane_sum_inverts(plane)) else plane
    return tuple((tuple(pts), W.shoelace2(pts), W.bounding_rect(pts)) for pts in W.find_external_contours(p != 0))


def row_reference(row):
    return [wire_ref_contours(tuple(s), row["sums"]) for s in row["planes"]]


@pytest.mark.parametrize("row", ALL_ROWS, ids=lambda r: r["id"])
def test_wire_ref_satisfies_every_rule_on_every_row(row):
    total = 0
    for n, (spec, ref) in enumerate(zip(row["planes"], row_reference(row))):
        plane = build_plane(spec)
        assert plane.shape == plane_shape(spec) and plane.dtype == np.uint8, (n, spec)
        fg = foreground(plane, row["sums"])
        assert np.array_equal(fg, (255 - plane if (row["sums"] and W.plane_sum_inverts(plane)) else plane) != 0), (n, spec)
        assert check_plane(fg, list(ref)) == [], (n, spec, check_plane(fg, list(ref))[:3])
        total += len(ref)
    if row["id"].startswith("empty"):
        assert total == 0


def test_the_rows_reach_the_edges_they_are_there_for():
    by = {r["id"]: r for r in ALL_ROWS}
    lat = wire_ref_contours(("lattice", 9, 129), False)
    assert len(lat) == 5 * 65 == ((9 + 1) // 2) * ((129 + 1) // 2) and all(len(p) == 1 and a == 0 for p, a, _ in lat)      # the root capacity, exactly
    a, b = build_plane(("inv127",)), build_plane(("inv127_plus1",))
    assert int(a.astype(np.int64).sum()) == 127 * 15 * 17 and not plane_inverts(a)                     # equality does not invert
    assert int(b.astype(np.int64).sum()) == 127 * 15 * 17 + 1 and plane_inverts(b) and int((a != b).sum()) == 1
    assert foreground(b)[b == 1].all() and foreground(b)[b == 0].all() and not foreground(b)[b == 255].any()
    inv = [plane_inverts(build_plane(s)) for s in by["inversion"]["planes"]]
    assert inv == [False, True, False, True, False, True], inv
    lo, hi = build_plane(by["inversion"]["planes"][2]), build_plane(by["inversion"]["planes"][3])
    assert lo.min() >= 1 and hi.max() <= 254 and foreground(lo).all() and foreground(hi).all()         # values in 1..254 are foreground under both rules
    for rid in ("lds_64k_no_optin", "lds_64k_plus_optin", "lds_160k_exact", "global_160k_plus"):
        assert len(wire_ref_contours(by[rid]["planes"][-1], False)) == -(-plane_shape(by[rid]["planes"][-1])[0] // 7), rid
    assert len(wire_ref_contours(by["lds_160k_exact"]["planes"][-1], False)) == 5852
    assert len(wire_ref_contours(by["grid_stride_513x512"]["planes"][0], False)) > 1000
    last = wire_ref_contours(by["plane_max_plus_1"]["planes"][-1], True)
    assert len(last) > 10 and any(len(p) > 4 for p, _, _ in last)                                       # the 33rd plane is not trivial
    assert max(len(p) for p, _, _ in wire_ref_contours(("comb", 23, 61), True)) > 100
    assert len(wire_ref_contours(("serpentine", 21, 37), True)) == 1
    from test_wires_gpu import _rings
    assert np.array_equal(build_plane(("rings",)), _rings())                                            # the plane the older contour test nests its rings on


# ---- answers stated by hand ------------------------------------------------------------------------------------------------------------
def _blank(h, w):
    return np.zeros((h, w), np.uint8)


def _known():
    out = []
    m = _blank(7, 9)
    m[2:5, 3:8] = 255
    out.append(("filled rectangle", m, [([(3, 2), (3, 4), (7, 4), (7, 2)], -16, (3, 2, 5, 3))]))
    m = _blank(5, 6)
    m[3, 4] = 255
    out.append(("one pixel", m, [([(4, 3)], 0, (4, 3, 1, 1))]))
    m = _blank(7, 9)
    m[3, 2:7] = 255
    out.append(("horizontal", m, [([(2, 3), (6, 3)], 0, (2, 3, 5, 1))]))
    m = _blank(7, 9)
    m[1:6, 4] = 255
    out.append(("vertical", m, [([(4, 1), (4, 5)], 0, (4, 1, 1, 5))]))
    m = _blank(7, 9)
    m[1, 2] = m[2, 3] = m[3, 4] = 255
    out.append(("diagonal", m, [([(2, 1), (4, 3)], 0, (2, 1, 3, 3))]))
    m = _blank(7, 9)
    m[1, 5] = m[2, 4] = m[3, 3] = 255
    out.append(("anti-diagonal", m, [([(5, 1), (3, 3)], 0, (3, 1, 3, 3))]))
    m = _blank(7, 9)
    m[1:6, 1:7] = 255
    m[2:5, 2:6] = 0
    m[3, 3] = 255
    out.append(("ring with a dot in its hole", m, [([(1, 1), (1, 5), (6, 5), (6, 1)], -40, (1, 1, 6, 5))]))
    out.append(("diagonal leak", build_plane(("leak",)), [([(2, 1), (1, 2), (1, 7), (8, 7), (8, 1)], -83, (1, 1, 8, 7))]))
    return out


@pytest.mark.parametrize("case", _known(), ids=lambda c: c[0])
def test_known_answers(case):
    name, m, want = case
    fg = m != 0
    assert check_plane(fg, want) == [], check_plane(fg, want)
    got = [(pts, W.shoelace2(pts), W.bounding_rect(pts)) for pts in W.find_external_contours(fg)]
    assert got == want, (name, got)
    assert len(external_components(fg)) == len(want)


def test_the_diagonal_leak_is_a_hole_because_the_background_is_4_connected():
    m = build_plane(("leak",))
    assert m[1, 1] == 0 and m[2, 2] == 0 and m[1, 2] and m[2, 1]                                       # outside and hole touch only across this diagonal
    comps = external_components(m != 0)
    assert len(comps) == 1 and comps[0][0] == (2, 1)
    m[2, 1] = 0                                                                                          # open the ring: the dot is outside now
    assert [c[0] for c in external_components(m != 0)] == [(2, 1), (4, 4)]


# ---- mutants of a correct answer ---------------------------------------------------------------------------------------------------------
def _base():
    m = _blank(12, 20)
    m[1:4, 2:7] = 255                                                                                    # A: a 5 x 3 rectangle
    m[5:11, 9:16] = 255                                                                                  # B: a ring ...
    m[6:10, 10:15] = 0
    m[8, 12] = 255                                                                                       # ... with a dot in its hole
    A = ([(2, 1), (2, 3), (6, 3), (6, 1)], -16, (2, 1, 5, 3))
    B = ([(9, 5), (9, 10), (15, 10), (15, 5)], -60, (9, 5, 7, 6))
    return m != 0, A, B


def _with_points(c, pts):
    return (pts, shoelace2(pts), c[2])


def _mutants():
    fg, A, B = _base()
    return fg, [B, A], {
        "a dropped vertex": ([B, _with_points(A, [(2, 1), (6, 3), (6, 1)])], {"segment"}),
        "the start rotated by one point": ([B, _with_points(A, [(2, 3), (6, 3), (6, 1), (2, 1)])], {"start"}),
        "reversed point order": ([B, _with_points(A, [(2, 1), (6, 1), (6, 3), (2, 3)])], {"orientation"}),
        "two contours swapped": ([A, B], {"order"}),
        "one point moved by one pixel": ([B, _with_points(A, [(2, 1), (2, 3), (7, 3), (6, 1)])], {"segment"}),
        "a rectangle one too wide": ([B, (A[0], A[1], (2, 1, 6, 3))], {"rect"}),
        "area2 negated": ([B, (A[0], 16, A[2])], {"area"}),
        "an internal component's contour added": ([([(12, 8)], 0, (12, 8, 1, 1)), B, A], {"count"}),
        "a collinear point inserted": ([B, _with_points(A, [(2, 1), (2, 2), (2, 3), (6, 3), (6, 1)])], {"collinear"}),
        "one side pushed out by a pixel": ([B, ([(2, 1), (2, 3), (7, 3), (7, 1)], -20, (2, 1, 6, 3))], {"border", "rect"}),
        "a pixel reported as a longer run": ([B, ([(2, 1), (6, 1)], 0, (2, 1, 5, 3))], {"border"}),
    }


def test_the_base_answer_is_correct_and_equals_wire_ref():
    fg, good, _ = _mutants()
    assert check_plane(fg, good) == []
    assert [(pts, W.shoelace2(pts), W.bounding_rect(pts)) for pts in W.find_external_contours(fg)] == good


@pytest.mark.parametrize("name", sorted(_mutants()[2]))
def test_each_mutant_is_rejected_under_the_rule_it_breaks(name):
    fg, _, mutants = _mutants()
    contours, rules = mutants[name]
    got = check_plane(fg, contours)
    assert {r for r, _, _ in got} == rules, (name, got)
    assert rules <= set(RULES)


def test_a_many_point_component_reported_as_one_point_breaks_the_single_rule():
    fg, A, B = _base()
    assert "single" in {r for r, _, _ in check_plane(fg, [B, ([(2, 1)], 0, A[2])])}
    m = _blank(3, 3)
    m[1, 1] = 255
    assert {r for r, _, _ in check_plane(m != 0, [([(1, 1), (1, 1)], 0, (1, 1, 1, 1))])} >= {"single", "segment"}


# ---- the one-channel resize of node_prepare --------------------------------------------------------------------------------------------
# measured on the planes of PREPARE_ROWS (emptied, then resized to height 12); exact integer arithmetic on fixed inputs, so asserted without margin
RESIZE_MAX_DEVIATION = 0.7671568627447556      # grey levels, against the float64 value before rounding
RESIZE_MAX_LEVELS = 1                          # against the float64 value rounded to the nearest integer


def _resize_deviation():
    worst, levels = 0.0, 0
    for row in PREPARE_ROWS:
        for (h, w, seed), kind in zip(row["planes"], row["boxes"]):
            e = W.empty_boxes(prepare_plane(h, w, seed), prepare_boxes(kind, h, w))
            nw = W.new_width(h, w, PREPARE_HEIGHT)
            fixed = resize_linear_u8(e[..., None], nw, PREPARE_HEIGHT)[..., 0].astype(np.float64)
            real = resize_bilinear_f64(e, nw, PREPARE_HEIGHT)
            worst = max(worst, float(np.abs(fixed - real).max()))
            levels = max(levels, int(np.abs(fixed - np.rint(real)).max()))
    return worst, levels


def test_fixed_point_resize_against_float64_on_the_prepare_rows():
    """oracle.preprocess.resize_linear_u8 (11-bit coefficients from a float32 coordinate, two truncating shifts, + 2 >> 2) against a float64
    half-pixel-centre bilinear resize that is not rounded, on every plane of PREPARE_ROWS (emptied, then resized to height 12).  Measured: the
    largest deviation is 0.7671568627447556 grey levels (the two truncating shifts and the 11-bit coefficients), and 1 level against the float64
    result rounded to the nearest integer.  Both are exact arithmetic on fixed inputs, so they are asserted as measured."""
    worst, levels = _resize_deviation()
    print(f"resize_linear_u8 vs float64 bilinear on the prepare rows: max |fixed - real| = {worst!r}, against the rounded value {levels} level(s)")
    assert worst <= RESIZE_MAX_DEVIATION and levels == RESIZE_MAX_LEVELS, (worst, levels)


def test_prepare_rows_are_well_formed():
    ids = [r["id"] for r in PREPARE_ROWS]
    assert len(ids) == len(set(ids))
    by = {r["id"]: r for r in PREPARE_ROWS}
    for r in PREPARE_ROWS:
        assert len(r["planes"]) == len(r["boxes"]) and set(r["boxes"]) <= {"kinds", "none"}, r["id"]
        assert all(W.new_width(h, w, PREPARE_HEIGHT) > 0 for h, w, _ in r["planes"]), r["id"]
    (h, w, _), = by["identity_12x18"]["planes"]
    assert h == PREPARE_HEIGHT and W.new_width(h, w, PREPARE_HEIGHT) == w
    (h, w, _), = by["down_2x_24x36"]["planes"]
    assert (h, w) == (2 * PREPARE_HEIGHT, 2 * W.new_width(h, w, PREPARE_HEIGHT))
    assert by["up_from_5x7"]["planes"][0][0] == 5 and W.new_width(5, 7, PREPARE_HEIGHT) > 7
    assert all(W.new_width(h, w, PREPARE_HEIGHT) == 0 for h, w in PREPARE_REFUSED)
    many = by["plane_max_plus_1"]
    assert len(many["planes"]) == 33 and [k for k, b in enumerate(many["boxes"]) if b != "none"] == [31, 32]
    # every box kind empties something somewhere, and the preserved ones nothing
    for r in PREPARE_ROWS:
        for (h, w, seed), kind in zip(r["planes"], r["boxes"]):
            p = prepare_plane(h, w, seed)
            e = W.empty_boxes(p, prepare_boxes(kind, h, w))
            assert (kind == "none") == np.array_equal(e, p), (r["id"], h, w)
