"""Numpy restatement of the reference's node-analysis front end.  TEST INFRASTRUCTURE ONLY (slow, per pixel / per border step).

CircuitAnalyzer.get_node_connections (/root/reference/src/circuit_analyzer.py:1286-1370) on the cropped SAM mask:
  1. empty the boxes of every class outside ('crossover', 'junction', 'circuit', 'vss')       :1327-1345
  2. resize_image_keep_aspect(new_height=600) + resize_bboxes                                  :787-809, :461-477
  3. enhance_lines: GaussianBlur((5,5), 1) -> dilate(ones(3,3), 2) -> erode(ones(3,3), 2)      :289-311
  4. get_contours(area_threshold=0.0004): findContours(RETR_EXTERNAL, CHAIN_APPROX_SIMPLE)      :388-459

OpenCV is not installed, so nothing here is pinned against cv2 itself.  Items marked [UP] (unpinned) restate documented OpenCV rules:
  [UP] the bit-exact 8-bit GaussianBlur (getGaussianKernelBitExact in ufixedpoint16, row then column pass, (s + 32768) >> 16)
  [UP] the point order of a traced border (icvFetchContour) and the list order of the contours (reverse raster order of the start
       pixels: cvFindContours inserts each new contour at the head of its list)
Everything else is exact integer arithmetic with independent checks in scipy (tests/test_wires_cpu.py).  The traced borders are judged by
geometry alone, without following a border, in tests/contour_ref.py (tests/test_contour_ref_cpu.py).
"""
import math

import numpy as np
from scipy import ndimage as ndi

from oracle.preprocess import resize_linear_u8

PRESERVED = ("crossover", "junction", "circuit", "vss")

# icvCodeDeltas: direction code s -> (dx, dy); 0 = right, 1 = up-right, 2 = up, 3 = up-left, 4 = left, 5 = down-left, 6 = down, 7 = down-right
DIRS = ((1, 0), (1, -1), (0, -1), (-1, -1), (-1, 0), (-1, 1), (0, 1), (1, 1))


# ---- 1 + 2: mask preparation ---------------------------------------------------------------------------------------------------------
def empty_boxes(mask, bboxes):
    """circuit_analyzer.py:1327-1345 on a copy."""
    m = mask.copy()
    H, W = m.shape[:2]
    for b in bboxes:
        if b["class"] not in PRESERVED:
            y0, y1 = max(0, int(b["ymin"])), min(H, int(b["ymax"]))
            x0, x1 = max(0, int(b["xmin"])), min(W, int(b["xmax"]))
            if y0 < y1 and x0 < x1:
                m[y0:y1, x0:x1] = 0
    return m


def new_width(H, W, new_height=600):
    return int(new_height * (W / H))                                   # resize_image_keep_aspect :799-803 (python float64)


def resize_keep_aspect(mask, bboxes, new_height=600):
    """circuit_analyzer.py:787-809 + resize_bboxes :461-477."""
    H, W = mask.shape[:2]
    nw = new_width(H, W, new_height)
    out = resize_linear_u8(mask[..., None], nw, new_height)[..., 0]
    sx, sy = nw / W, new_height / H
    bb = []
    for b in bboxes:
        r = dict(b)
        r["xmin"], r["ymin"] = int(b["xmin"] * sx), int(b["ymin"] * sy)
        r["xmax"], r["ymax"] = int(b["xmax"] * sx), int(b["ymax"] * sy)
        bb.append(r)
    return out, bb


# ---- 3: enhance_lines ----------------------------------------------------------------------------------------------------------------
def gaussian_kernel_bitexact(n=5, sigma=1.0):
    """[UP] getGaussianKernelBitExact in ufixedpoint16 (8 fractional bits): off-centre taps cvRound(256 e^{-d^2 / (2 sigma^2)} / sum),
    the centre tap takes 256 - the others (the taps of a symmetric kernel sum to exactly 1.0)."""
    c = n // 2
    e = [math.exp(-((i - c) ** 2) / (2.0 * sigma * sigma)) for i in range(n)]
    s = sum(e)
    k = [int(np.rint(256.0 * v / s)) for v in e]                      # cvRound: round half to even on a double
    k[c] = 256 - (sum(k) - k[c])
    return np.array(k, dtype=np.int64)


def reflect101(p, n):
    """cv::borderInterpolate(BORDER_REFLECT_101); a plane 1 pixel long maps everything to 0."""
    if n == 1:
        return 0
    while p < 0 or p >= n:
        p = -p if p < 0 else 2 * n - 2 - p
    return p


def gaussian_blur_5x5(img):
    """[UP] cv2.GaussianBlur(img, (5,5), 1) on u8: row pass, column pass, (sum + 32768) >> 16, BORDER_REFLECT_101."""
    H, W = img.shape
    k = gaussian_kernel_bitexact()
    xi = np.array([[reflect101(x + d, W) for d in range(-2, 3)] for x in range(W)])
    yi = np.array([[reflect101(y + d, H) for d in range(-2, 3)] for y in range(H)])
    src = img.astype(np.int64)
    rows = (src[:, xi] * k[None, None, :]).sum(-1)                    # [H, W]
    cols = (rows[yi] * k[None, :, None]).sum(1)                       # [H, W]
    return ((cols + 32768) >> 16).astype(np.uint8)


def _rank_filter5(img, fn):
    """5 x 5 max / min with the border replicated (cv2.dilate / erode with the default border value = pixels outside are ignored)."""
    H, W = img.shape
    p = np.pad(img, 2, mode="edge")
    out = p[2:2 + H, 2:2 + W].copy()
    for dy in range(5):
        for dx in range(5):
            out = fn(out, p[dy:dy + H, dx:dx + W])
    return out


def dilate2(img):
    return _rank_filter5(img, np.maximum)                             # cv2.dilate(ones(3,3), iterations=2) = one 5 x 5 rectangle


def erode2(img):
    return _rank_filter5(img, np.minimum)


def enhance_lines(img):
    """circuit_analyzer.py:289-311."""
    return erode2(dilate2(gaussian_blur_5x5(img)))


# ---- 4: get_contours -----------------------------------------------------------------------------------------------------------------
def external_roots(fg):
    """Raster-first pixel (x, y) of every 8-connected foreground component that lies in no hole of another component (the background,
    4-connected, padded with a one-pixel zero frame, is the outer one at the root's left neighbour), in raster order."""
    H, W = fg.shape
    lab, n = ndi.label(fg, structure=np.ones((3, 3), bool))
    if n == 0:
        return []
    flat = lab.ravel()
    ids, first = np.unique(flat, return_index=True)
    first = first[ids > 0]
    bg = np.pad(~fg, 1, constant_values=True)
    blab, _ = ndi.label(bg)                                           # 4-connectivity
    outer = blab[0, 0]
    roots = []
    for idx in np.sort(first):
        y, x = divmod(int(idx), W)
        if blab[y + 1, x] == outer:                                   # left neighbour, in padded coordinates
            roots.append((x, y))
    return roots


def trace_border(fg, x0, y0):
    """[UP] icvFetchContour with CHAIN_APPROX_SIMPLE from an outer-border start pixel: -> list of (x, y) points."""
    H, W = fg.shape

    def nz(x, y):
        return 0 <= x < W and 0 <= y < H and bool(fg[y, x])
    s = 4
    while True:                                                        # first neighbour: s = 3, 2, 1, 0, 7, 6, 5 (4 = the start's left)
        s = (s - 1) & 7
        x1, y1 = x0 + DIRS[s][0], y0 + DIRS[s][1]
        if nz(x1, y1) or s == 4:
            break
    if s == 4:
        return [(x0, y0)]
    pts = []
    x3, y3 = x0, y0
    prev_s = s ^ 4
    while True:
        s_end = s
        while True:                                                    # counter-clockwise from back + 1
            s += 1
            x4, y4 = x3 + DIRS[s & 7][0], y3 + DIRS[s & 7][1]
            if nz(x4, y4) or s >= 15:
                break
        s &= 7
        if s != prev_s:
            pts.append((x3, y3))
            prev_s = s
        if (x4, y4) == (x0, y0) and (x3, y3) == (x1, y1):
            break
        x3, y3 = x4, y4
        s = (s + 4) & 7
    return pts


def shoelace2(pts):
    """2 x the signed area of the closed polygon (exact integer)."""
    a = 0
    n = len(pts)
    for i in range(n):
        xa, ya = pts[i - 1]
        xb, yb = pts[i]
        a += xa * yb - xb * ya
    return a


def bounding_rect(pts):
    xs = [p[0] for p in pts]
    ys = [p[1] for p in pts]
    return (min(xs), min(ys), max(xs) - min(xs) + 1, max(ys) - min(ys) + 1)


def find_external_contours(fg):
    """findContours(RETR_EXTERNAL, CHAIN_APPROX_SIMPLE) on a binary plane: list of point lists, [UP] in reverse raster order of their
    start pixels."""
    return [trace_border(fg, x, y) for x, y in reversed(external_roots(fg))]


def plane_sum_inverts(img):
    """cv2.mean(img)[0] > 127, in integers."""
    return int(img.astype(np.int64).sum()) > 127 * img.shape[0] * img.shape[1]


def get_contours(img, area_threshold=0.00040):
    """circuit_analyzer.py:388-459 without the drawing: -> (contour dicts, zero canvas).  Mutates `img` as the reference does
    (img[img == 255] = 1) when there is no inversion."""
    if plane_sum_inverts(img):
        img = 255 - img
    img[img == 255] = 1
    H, W = img.shape
    norm = H * W
    out = []
    for pts in find_external_contours(img != 0):
        area = abs(shoelace2(pts)) / 2.0
        if area / norm > area_threshold:
            out.append({"id": len(out), "contour": np.array(pts, dtype=np.int32).reshape(-1, 1, 2), "area": area / norm,
                        "rectangle": bounding_rect(pts)})
    return out, np.zeros((H, W, 3), dtype=np.uint8)


def node_contours(mask, bboxes, new_height=600, area_threshold=0.0004):
    """Steps 1-4 for one image: -> (emptied mask, resized boxes, enhanced plane as get_contours leaves it, contour dicts)."""
    emptied = empty_boxes(mask, bboxes)
    resized, rb = resize_keep_aspect(emptied, bboxes, new_height)
    enhanced = enhance_lines(resized)
    contours, _ = get_contours(enhanced, area_threshold)
    return emptied, rb, enhanced, contours


def wire_mask(img):
    """A 0 / 255 wire mask from a synth.circuit_image (dark strokes = wires)."""
    return np.where(img.min(axis=2) < 128, 255, 0).astype(np.uint8)
