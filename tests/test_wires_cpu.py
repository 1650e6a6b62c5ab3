"""The node-analysis reference (tests/wire_ref.py) against hand-derived answers and independent scipy checks.  No GPU."""
import numpy as np
import pytest
from scipy import ndimage as ndi

import wire_ref as W
from synth import circuit_image


def _plane(h, w, pts=(), rects=()):
    m = np.zeros((h, w), np.uint8)
    for x, y in pts:
        m[y, x] = 255
    for x0, y0, x1, y1 in rects:
        m[y0:y1 + 1, x0:x1 + 1] = 255
    return m


def _contours(m):
    return W.find_external_contours(m != 0)


# ---- known answers by hand -----------------------------------------------------------------------------------------------------
def test_gaussian_taps_derive_to_opencv_bitexact_values():
    assert W.gaussian_kernel_bitexact().tolist() == [14, 63, 102, 63, 14]
    assert W.gaussian_kernel_bitexact().sum() == 256


def test_filled_rectangle_point_order_and_area():
    m = _plane(20, 30, rects=[(4, 3, 12, 9)])
    (c,) = _contours(m)
    assert c == [(4, 3), (4, 9), (12, 9), (12, 3)]
    assert abs(W.shoelace2(c)) == 2 * (12 - 4) * (9 - 3)
    assert W.bounding_rect(c) == (4, 3, 9, 7)


def test_single_pixel_gives_one_point():
    assert _contours(_plane(5, 5, pts=[(2, 3)])) == [[(2, 3)]]


def test_segments_give_their_end_points_and_zero_area():
    (h,) = _contours(_plane(10, 10, rects=[(2, 4, 7, 4)]))
    assert h == [(2, 4), (7, 4)] and W.shoelace2(h) == 0
    (v,) = _contours(_plane(10, 10, rects=[(3, 1, 3, 6)]))
    assert v == [(3, 1), (3, 6)] and W.shoelace2(v) == 0
    (d,) = _contours(_plane(10, 10, pts=[(1 + i, 2 + i) for i in range(5)]))
    assert d == [(1, 2), (5, 6)] and W.shoelace2(d) == 0


def test_diagonally_touching_pixels_are_one_contour():
    cs = _contours(_plane(6, 6, pts=[(2, 2), (3, 3)]))
    assert cs == [[(2, 2), (3, 3)]]
    cs = _contours(_plane(6, 6, pts=[(3, 2), (2, 3)]))
    assert cs == [[(3, 2), (2, 3)]]


def test_ring_with_a_dot_inside_excludes_the_dot():
    m = _plane(20, 20, rects=[(2, 2, 14, 2), (2, 14, 14, 14), (2, 2, 2, 14), (14, 2, 14, 14)], pts=[(8, 8)])
    cs = _contours(m)
    assert len(cs) == 1 and cs[0] == [(2, 2), (2, 14), (14, 14), (14, 2)]


def test_components_touching_each_edge():
    m = _plane(12, 16, rects=[(0, 4, 2, 6), (13, 5, 15, 7), (6, 0, 8, 1), (6, 10, 9, 11)])
    cs = _contours(m)
    starts = sorted(c[0] for c in cs)
    assert len(cs) == 4 and sorted([(6, 0), (0, 4), (13, 5), (6, 10)]) == starts
    for c in cs:
        assert all(0 <= x < 16 and 0 <= y < 12 for x, y in c)


def test_reverse_raster_order_of_start_pixels():
    m = _plane(10, 10, pts=[(1, 1), (7, 1), (4, 5), (0, 8)])
    cs = _contours(m)
    assert [c[0] for c in cs] == [(0, 8), (4, 5), (7, 1), (1, 1)]


def test_enhance_known_answers():
    assert (W.enhance_lines(np.zeros((7, 9), np.uint8)) == 0).all()
    assert (W.enhance_lines(np.full((3, 4), 200, np.uint8)) == 200).all()
    one = np.array([[77]], np.uint8)
    assert W.gaussian_blur_5x5(one)[0, 0] == 77                      # 1 x 1: every tap reads index 0


# ---- scipy cross-checks ------------------------------------------------------------------------------------------------------------
def _planes():
    rng = np.random.default_rng(5)
    out = [rng.integers(0, 256, (h, w), dtype=np.uint8) for h, w in ((1, 1), (1, 7), (7, 1), (5, 6), (37, 71))]
    out += [np.where(rng.random((40, 50)) < 0.3, 255, 0).astype(np.uint8)]
    out += [W.wire_mask(circuit_image(120, 160, seed=s)) for s in (1, 2)]
    return out


@pytest.mark.parametrize("i", range(8))
def test_dilate_erode_equal_scipy_grey_filters(i):
    x = _planes()[i]
    assert np.array_equal(W.dilate2(x), ndi.grey_dilation(x, size=5, mode="nearest"))
    assert np.array_equal(W.erode2(x), ndi.grey_erosion(x, size=5, mode="nearest"))


@pytest.mark.parametrize("i", range(3, 8))
def test_blur_equals_scipy_with_the_fixed_point_taps_and_is_near_the_float_gaussian(i):
    """scipy's separable filter (mode='mirror' = REFLECT_101) with the 8-bit taps / 256, rounded half up, is the blur exactly; the float64
    Gaussian itself differs from it only by the tap quantisation (|tap error| <= 0.0042, so <= 2 grey levels on u8 content)."""
    x = _planes()[i]                                                 # (planes >= 3 wide: scipy's mirror differs from REFLECT_101 below)
    got = W.gaussian_blur_5x5(x).astype(np.float64)

    def sep(k):
        return ndi.correlate1d(ndi.correlate1d(x.astype(np.float64), k, axis=0, mode="mirror"), k, axis=1, mode="mirror")
    assert np.array_equal(got, np.floor(sep(W.gaussian_kernel_bitexact() / 256.0) + 0.5))
    k = np.exp(-np.arange(-2, 3) ** 2 / 2.0)
    d = np.abs(got - sep(k / k.sum()))
    assert d.max() <= 2.0, d.max()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_contours_match_filled_components_and_rectangles(seed):
    rng = np.random.default_rng(seed)
    planes = [np.where(rng.random((60, 80)) < 0.45, 255, 0).astype(np.uint8),
              W.enhance_lines(W.wire_mask(circuit_image(150, 200, seed=seed)))]
    for m in planes:
        fg = m != 0
        cs = _contours(m)
        lab, n = ndi.label(ndi.binary_fill_holes(fg), structure=np.ones((3, 3), bool))
        assert len(cs) == n
        want = sorted((s[1].start, s[0].start, s[1].stop - s[1].start, s[0].stop - s[0].start) for s in ndi.find_objects(lab))
        assert sorted(W.bounding_rect(c) for c in cs) == want


def test_emptying_and_area_filter_and_in_place_binarization():
    m = np.full((40, 60), 255, np.uint8)
    m[10:30, 10:50] = 0
    boxes = [{"class": "resistor", "xmin": 5.7, "ymin": -3, "xmax": 20.2, "ymax": 8},
             {"class": "junction", "xmin": 30, "ymin": 30, "xmax": 40, "ymax": 40},
             {"class": "capacitor", "xmin": 70, "ymin": 0, "xmax": 90, "ymax": 10}]
    e = W.empty_boxes(m, boxes)
    want = m.copy()
    want[0:8, 5:20] = 0
    assert np.array_equal(e, want)
    # mostly white -> inverted, the caller's array stays as it was
    img = np.where(np.arange(100)[None, :] < 80, 255, 0).astype(np.uint8).repeat(10, 0)
    before = img.copy()
    cs, canvas = W.get_contours(img)
    assert np.array_equal(img, before) and canvas.shape == (10, 100, 3) and not canvas.any()
    assert len(cs) == 1 and cs[0]["rectangle"] == (80, 0, 20, 10)
    # not inverted -> 255 becomes 1 in place; a 2 x 2 blob is below the area threshold, a 10 x 10 one is above
    img = _plane(100, 100, rects=[(5, 5, 6, 6), (50, 50, 59, 59)])
    cs, _ = W.get_contours(img)
    assert set(np.unique(img).tolist()) == {0, 1}
    assert [c["rectangle"] for c in cs] == [(50, 50, 10, 10)] and cs[0]["id"] == 0
    assert cs[0]["area"] == 81 / 10000 and cs[0]["contour"].dtype == np.int32 and cs[0]["contour"].shape == (4, 1, 2)


def test_resize_keep_aspect_boxes_and_width():
    m = np.zeros((300, 451), np.uint8)
    out, bb = W.resize_keep_aspect(m, [{"class": "r", "xmin": 10, "ymin": 11, "xmax": 100, "ymax": 299}])
    assert out.shape == (600, int(600 * (451 / 300)))
    sx = out.shape[1] / 451
    assert bb[0]["xmin"] == int(10 * sx) and bb[0]["ymin"] == 22 and bb[0]["ymax"] == 598
