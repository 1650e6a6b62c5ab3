"""A geometric oracle for findContours(RETR_EXTERNAL, CHAIN_APPROX_SIMPLE), independent of the border trace.  TEST INFRASTRUCTURE ONLY.

tests/wire_ref.py restates icvFetchContour step by step, and so does trace_border in wire_ops.hip: a misreading shared by the two would pass a
bit-for-bit comparison.  This module never follows a border.  It works from the foreground plane with numpy and scipy alone and states what
any correct answer must satisfy:

  * scipy labels the foreground 8-connected and the background 4-connected after a one-pixel background frame was padded on;
  * a component is EXTERNAL when one of its pixels has a 4-neighbour in the frame's background set, and those pixels are its outer border;
  * check_plane(fg, contours) lists every rule the contours of one plane break (count, order, start, segment, collinear, border, rect, area,
    orientation, single); an empty list means they are correct.

It also builds the planes of op_matrix.CONTOUR_ROWS / PREPARE_ROWS from their specs (seeded: the rows are data) and holds the float64
bilinear resize the one-channel fixed-point resize is measured against."""
import functools

import numpy as np
from scipy import ndimage as ndi

RULES = ("count", "order", "start", "segment", "collinear", "border", "rect", "area", "orientation", "single")


# ---- the foreground and its external components --------------------------------------------------------------------------------------
def plane_inverts(plane):
    """get_contours' cv2.mean(img) > 127 in integers: the plane's sum exceeds 127 * H * W."""
    return int(plane.astype(np.int64).sum()) > 127 * plane.shape[0] * plane.shape[1]


def foreground(plane, sums_given=True):
    """v != 0, or v != 255 when the sums are given and the plane inverts."""
    return plane != 255 if (sums_given and plane_inverts(plane)) else plane != 0


def external_components(fg):
    """-> [(first (x, y), sorted outer-border pixel ids y * W + x, rect (x, y, w, h), number of pixels)] of the external components, in raster
    order of their raster-first pixels."""
    H, W = fg.shape
    lab, n = ndi.label(fg, structure=np.ones((3, 3), bool))
    if n == 0:
        return []
    blab, _ = ndi.label(np.pad(~fg, 1, constant_values=True))          # 4-connected; the frame is background
    outer = blab == blab[0, 0]
    near = outer[1:-1, :-2] | outer[1:-1, 2:] | outer[:-2, 1:-1] | outer[2:, 1:-1]
    ys, xs = np.nonzero(fg & near)
    ids = lab[ys, xs]
    order = np.argsort(ids, kind="stable")                              # nonzero is in raster order: each group stays sorted by pixel id
    ids, pix = ids[order], (ys * W + xs)[order]
    cuts = np.flatnonzero(np.diff(ids)) + 1
    groups = dict(zip(ids[np.concatenate(([0], cuts))].tolist(), np.split(pix, cuts))) if len(ids) else {}
    labels, first = np.unique(lab.ravel(), return_index=True)
    sizes = np.bincount(lab.ravel())
    boxes = ndi.find_objects(lab)
    out = []
    for k, f in zip(labels.tolist(), first.tolist()):
        if k == 0 or k not in groups:
            continue
        sy, sx = boxes[k - 1]
        out.append(((f % W, f // W), groups[k], (sx.start, sy.start, sx.stop - sx.start, sy.stop - sy.start), int(sizes[k])))
    out.sort(key=lambda c: c[0][1] * W + c[0][0])
    return out


# ---- the rules -----------------------------------------------------------------------------------------------------------------------------
def _sgn(v):
    return (v > 0) - (v < 0)


def shoelace2(pts):
    """2 x the signed area of the closed polygon, in python integers."""
    a = 0
    for i in range(len(pts)):
        (xa, ya), (xb, yb) = pts[i - 1], pts[i]
        a += xa * yb - xb * ya
    return a


def _segment_pixels(pts, W):
    """Pixel ids on the closing-inclusive segments (only called once every segment is horizontal, vertical or 45 degrees)."""
    out = []
    for i in range(len(pts)):
        (xa, ya), (xb, yb) = pts[i - 1], pts[i]
        n = max(abs(xb - xa), abs(yb - ya))
        t = np.arange(n + 1)
        out.append((ya + _sgn(yb - ya) * t) * W + xa + _sgn(xb - xa) * t)
    return np.unique(np.concatenate(out))


def check_plane(fg, contours):
    """contours: [(points [n, 2] as (x, y), 2 x signed area, rect (x, y, w, h))] of one plane, in the order they were returned.
    -> [(rule, contour position, detail)], empty when the contours are the plane's external contours."""
    H, W = fg.shape
    comps = external_components(fg)
    bad = []
    if len(contours) != len(comps):
        return [("count", -1, f"{len(contours)} contours for {len(comps)} external components")]
    want = comps[::-1]                                                   # reverse raster order of the raster-first pixels
    by_start = {c[0]: c for c in comps}
    for k, (pts, area2, rect) in enumerate(contours):
        pts = [(int(x), int(y)) for x, y in np.asarray(pts).reshape(-1, 2).tolist()]
        comp = want[k]
        if not pts:
            bad.append(("start", k, "no points"))
            continue
        if pts[0] != comp[0]:
            if pts[0] in by_start:
                bad.append(("order", k, f"starts at {pts[0]}, the component due here starts at {comp[0]}"))
                comp = by_start[pts[0]]
            else:
                bad.append(("start", k, f"starts at {pts[0]}, not at the raster-first pixel {comp[0]}"))
        first, border, box, size = comp
        n = len(pts)
        if (size == 1) != (n == 1) or (n == 1 and int(area2) != 0):
            bad.append(("single", k, f"{n} points, area {int(area2)} for a component of {size} pixels"))
        dirs = [(_sgn(pts[i][0] - pts[i - 1][0]), _sgn(pts[i][1] - pts[i - 1][1])) for i in range(n)] if n > 1 else []
        straight = True
        for i in range(len(dirs)):
            dx, dy = pts[i][0] - pts[i - 1][0], pts[i][1] - pts[i - 1][1]
            if (dx == 0 and dy == 0) or (dx != 0 and dy != 0 and abs(dx) != abs(dy)):
                bad.append(("segment", k, f"{pts[i - 1]} -> {pts[i]} is not horizontal, vertical or diagonal"))
                straight = False
        for i in range(len(dirs)):
            if dirs[i] == dirs[(i + 1) % n]:
                bad.append(("collinear", k, f"point {i} {pts[i]} lies inside a straight run"))
        inside = all(0 <= x < W and 0 <= y < H for x, y in pts)
        if not inside:
            bad.append(("border", k, "a point outside the plane"))
        elif straight:
            got = _segment_pixels(pts, W) if n > 1 else np.array([pts[0][1] * W + pts[0][0]])
            if not np.array_equal(got, border):
                miss, extra = np.setdiff1d(border, got), np.setdiff1d(got, border)
                bad.append(("border", k, f"{len(miss)} outer-border pixels not on the segments, {len(extra)} segment pixels not on the outer border"))
        if tuple(int(v) for v in rect) != box:
            bad.append(("rect", k, f"{tuple(int(v) for v in rect)} != {box}"))
        a = shoelace2(pts)
        if int(area2) != a:
            bad.append(("area", k, f"{int(area2)} != the shoelace sum {a}"))
        if a > 0:
            bad.append(("orientation", k, f"the shoelace sum {a} is positive"))
    return bad


# ---- the planes of op_matrix.CONTOUR_ROWS --------------------------------------------------------------------------------------------
def rings(h=120, w=160):
    """Nested square rings with a dot in the middle, a filled rectangle, a ring with a dot in its hole (tests/test_wires_gpu.py's _rings())."""
    m = np.zeros((h, w), np.uint8)
    for k in range(0, 50, 6):
        m[10 + k, 10 + k:110 - k] = 255
        m[109 - k, 10 + k:110 - k] = 255
        m[10 + k:110 - k, 10 + k] = 255
        m[10 + k:110 - k, 109 - k] = 255
    m[59, 59] = 255
    m[5:20, 130:150] = 255
    m[50:70, 125:155] = 255
    m[55:65, 130:150] = 0
    m[60, 140] = 255
    return m


def diagonal_leak():
    """A ring whose hole reaches the outside only across a diagonal: the background is 4-connected, so the hole stays a hole and the dot in
    it is not external.  One external contour."""
    m = np.zeros((9, 11), np.uint8)
    m[1, 2:8] = 255
    m[7, 1:8] = 255
    m[2:8, 1] = 255                                                       # the corner (1, 1) stays open: it touches the hole pixel (2, 2) only diagonally
    m[1:8, 8] = 255
    m[4, 4] = 255
    return m


def comb(h=23, w=61):
    """A spine with teeth every other column: a long border with two vertices per tooth tip and per gap."""
    m = np.zeros((h, w), np.uint8)
    m[1, 1:w - 1] = 255
    m[1:h - 1, 1:w - 1:2] = 255
    return m


def serpentine(h=21, w=37):
    """A one-pixel-wide path that winds over the plane: the trace walks out along it and back over the same pixels."""
    m = np.zeros((h, w), np.uint8)
    for i, y in enumerate(range(1, h - 1, 2)):
        m[y, 1:w - 1] = 255
        if y + 2 < h - 1:
            m[y + 1, w - 2 if i % 2 == 0 else 1] = 255
    return m


def _inv127(plus_one):
    """15 x 17 = 255 pixels, exactly 127 of them at 255: the sum equals 127 * H * W and the plane does not invert; with one 0 turned to 1 it does."""
    m = np.zeros(255, np.uint8)
    m[np.random.default_rng(127).permutation(255)[:127]] = 255
    if plus_one:
        m[np.flatnonzero(m == 0)[40]] = 1
    return m.reshape(15, 17)


@functools.lru_cache(maxsize=None)
def _plane(spec):
    kind, a = spec[0], spec[1:]
    if kind == "rand":                                                    # (H, W, density, seed)
        return np.where(np.random.default_rng(a[3]).random((a[0], a[1])) < a[2], 255, 0).astype(np.uint8)
    if kind == "full":
        return np.full((a[0], a[1]), 255, np.uint8)
    if kind == "zero":
        return np.zeros((a[0], a[1]), np.uint8)
    if kind == "lastrc":                                                  # foreground only in the last column and the last row
        m = np.zeros((a[0], a[1]), np.uint8)
        m[-1, :] = 255
        m[:, -1] = 255
        return m
    if kind == "lattice":                                                 # isolated pixels at even (x, y): ceil(H / 2) * ceil(W / 2) contours
        m = np.zeros((a[0], a[1]), np.uint8)
        m[::2, ::2] = 255
        return m
    if kind == "values":                                                  # (H, W, seed, palette): every pixel drawn from the palette
        return np.random.default_rng(a[2]).choice(np.array(a[3], dtype=np.uint8), size=(a[0], a[1]))
    if kind == "stripes":                                                 # (H, W, cut): rows y % 7 < 4; `cut` removes some pixels of the last column
        m = np.zeros((a[0], a[1]), np.uint8)
        m[np.arange(a[0]) % 7 < 4, :] = 255
        if a[2]:
            m[np.arange(a[0]) % 5 == 1, -1] = 0
        return m
    fixed = {"rings": rings, "leak": diagonal_leak, "comb": comb, "serpentine": serpentine, "inv127": lambda: _inv127(False),
             "inv127_plus1": lambda: _inv127(True)}
    return fixed[kind]()


def build_plane(spec):
    """A fresh copy of the plane a row's spec names."""
    return _plane(tuple(spec)).copy()


# ---- the planes and boxes of op_matrix.PREPARE_ROWS -----------------------------------------------------------------------------------
def prepare_plane(h, w, seed):
    """Full-range u8 noise: zeros are rare, so an emptied box shows, and the resize has every value to round."""
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def prepare_boxes(kind, h, w):
    """The box kinds of tests/test_wires_gpu.py on an h x w plane."""
    if kind == "none":
        return []
    assert kind == "kinds", kind
    return [{"class": "resistor", "xmin": -15.5, "ymin": -3, "xmax": w / 4 + 0.9, "ymax": h / 3 + 0.2},        # negative
            {"class": "capacitor", "xmin": w - 2, "ymin": h - 1, "xmax": w + 50, "ymax": h + 99},            # past the edge
            {"class": "inductor", "xmin": w // 2, "ymin": 0, "xmax": w // 2, "ymax": h},                       # empty
            {"class": "junction", "xmin": 0, "ymin": 0, "xmax": w, "ymax": h},                                 # preserved
            {"class": "vss", "xmin": 0, "ymin": 0, "xmax": w // 2 + 1, "ymax": h // 2 + 1},                    # preserved
            {"class": "diode", "xmin": w // 3, "ymin": h // 4, "xmax": w // 2 + 1.7, "ymax": h // 2 + 1.2}]


# ---- the float64 yardstick of the one-channel resize ------------------------------------------------------------------------------------
def resize_bilinear_f64(img, dst_w, dst_h):
    """Half-pixel-centre bilinear resize of a [H, W] plane in float64, coordinates clamped to the plane, not rounded."""
    H, W = img.shape

    def axis(dst, src):
        f = (np.arange(dst, dtype=np.float64) + 0.5) * (src / dst) - 0.5
        f = np.clip(f, 0.0, src - 1.0)
        s = np.minimum(np.floor(f).astype(np.int64), max(src - 2, 0))
        return s, np.minimum(s + 1, src - 1), f - s
    x0, x1, fx = axis(dst_w, W)
    y0, y1, fy = axis(dst_h, H)
    v = img.astype(np.float64)
    top = v[y0][:, x0] * (1 - fx) + v[y0][:, x1] * fx
    bot = v[y1][:, x0] * (1 - fx) + v[y1][:, x1] * fx
    return top * (1 - fy)[:, None] + bot * fy[:, None]
