"""Numpy restatement of the reference's terminal reclassification.  TEST INFRASTRUCTURE ONLY.  Built on tests/wire_ref.py (get_contours) and
tests/node_ref.py (is_point_near_bbox).

CircuitAnalyzer.reclassify_terminals_based_on_connectivity (circuit_analyzer.py:2217-2311), which run_terminal_reclassification
(analysis_pipeline.py:117-137) calls between the segmenter and node analysis:
  1. cvtColor(RGB2BGR), then segment_circuit (:313-319): cvtColor(RGB2GRAY) on the swapped image -- the R weight falls on channel 2 of the
     method's input -- and adaptiveThreshold(255, ADAPTIVE_THRESH_MEAN_C, THRESH_BINARY_INV, 31, 21)
  2. every box whose class is outside ('crossover', 'junction', 'circuit', 'vss') is emptied with a numpy slice
     [max(0, ymin):min(H, ymax), max(0, xmin):min(W, xmax)] of int() coordinates -- no ymin < ymax guard, so a negative ymax / xmax counts
     from the end (:2244-2249)
  3. get_contours(area_threshold=0.0001) (:2254)
  4. every 'terminal' box against EVERY contour (no broad phase): connected when one contour point passes is_point_near_bbox(., ., 10)
  5. two or more connected contours: class -> 'voltage.dc', the old class kept in 'original_yolo_class_if_reclassified',
     '_yolo_class_id_temp' -> the id of 'voltage.dc' in the detector's names when it has one, 'was_reclassified_from_terminal' = True

OpenCV is not installed, so nothing here is pinned against cv2 itself.  [UP] (unpinned) items restate OpenCV 4's documented rules:
  [UP] RGB2Gray<uchar>: (R * 9798 + G * 19235 + B * 3735 + 16384) >> 15
  [UP] adaptiveThreshold's mean: boxFilter 31 x 31, normalised, BORDER_REPLICATE | BORDER_ISOLATED, u8 output cvRound(sum * (1 / 961.));
       961 is odd, so no sum is a tie and rint(S / 961) == (2 S + 961) // 1922 (tests/test_terminal_reclass_cpu.py checks every S)
  [UP] the threshold table tab[src - mean + 255] with idelta = cvFloor(21): 255 where src - mean <= -21, else 0
"""
import numpy as np

import node_ref as R
import wire_ref as W

PRESERVED = ("crossover", "junction", "circuit", "vss")
BLOCK, DELTA = 31, 21
NEAR = 10                                                             # pixel_threshold_for_reclass :2277
AREA = 0.0001


def grey(img, red_channel=0):
    """[UP] cvtColor(RGB2GRAY) on u8 [H, W, 3] with the R weight on channel `red_channel` (0 or 2) and the B weight on the other end."""
    x = img.astype(np.int64)
    return ((x[..., red_channel] * 9798 + x[..., 1] * 19235 + x[..., 2 - red_channel] * 3735 + 16384) >> 15).astype(np.uint8)


def box_sums(g, k=BLOCK):
    """Sum over the k x k neighbourhood of every pixel, the border replicated: an integral image of the edge-padded plane."""
    r = k // 2
    H, Wd = g.shape
    p = np.pad(g.astype(np.int64), r, mode="edge")
    ii = np.zeros((p.shape[0] + 1, p.shape[1] + 1), np.int64)
    ii[1:, 1:] = p.cumsum(0).cumsum(1)
    return ii[k:k + H, k:k + Wd] - ii[:H, k:k + Wd] - ii[k:k + H, :Wd] + ii[:H, :Wd]


def rounded_mean(s, k=BLOCK):
    """[UP] cvRound(S * (1 / k^2)) in integers (k odd: no ties)."""
    n = k * k
    return (2 * s + n) // (2 * n)


def adaptive_threshold(g, k=BLOCK, delta=DELTA):
    """[UP] adaptiveThreshold(g, 255, ADAPTIVE_THRESH_MEAN_C, THRESH_BINARY_INV, k, delta)."""
    return np.where(g.astype(np.int64) - rounded_mean(box_sums(g, k), k) <= -delta, 255, 0).astype(np.uint8)


def segment_circuit(img, red_channel=0):
    """circuit_analyzer.py:313-319 (red_channel = 0: the method called on its own)."""
    return adaptive_threshold(grey(img, red_channel))


def empty_boxes(mask, bboxes):
    """:2244-2249 on a copy, with numpy's own slicing."""
    m = mask.copy()
    H, Wd = m.shape
    for b in bboxes:
        if b.get("class") not in PRESERVED:
            ymin, ymax = int(b["ymin"]), int(b["ymax"])
            xmin, xmax = int(b["xmin"]), int(b["xmax"])
            m[max(0, ymin):min(H, ymax), max(0, xmin):min(Wd, xmax)] = 0
    return m


def voltage_dc_id(names):
    for num_id, name in (names.items() if hasattr(names, "items") else enumerate(names)):
        if name == "voltage.dc":
            return num_id
    return None


def reclassify(image, bboxes, names, red_channel=0, area_threshold=AREA):
    """Steps 1-5 on one u8 [H, W, 3] image with the R weight on `red_channel` (the reference's method: 2; the pipeline, which swaps once
    more before it calls the method: 0).  Rewrites `bboxes` in place.  -> ({box index: connected contours} of its terminals, emptied mask)."""
    mask = empty_boxes(segment_circuit(image, red_channel), bboxes)
    contours, _ = W.get_contours(mask.copy(), area_threshold)
    dc = voltage_dc_id(names)
    counts = {}
    for i, b in enumerate(bboxes):
        if b.get("class") != "terminal":
            continue
        n = sum(any(R.is_point_near_bbox(p, b, NEAR) for p in c["contour"].reshape(-1, 2)) for c in contours)
        counts[i] = n
        if n >= 2:
            b["original_yolo_class_if_reclassified"] = b["class"]
            b["class"] = "voltage.dc"
            if dc is not None:
                b["_yolo_class_id_temp"] = dc
            b["was_reclassified_from_terminal"] = True
    return counts, mask


# ---- the fixture's vocabulary (tests/golden/terminal_reclass.json) -----------------------------------------------------------------
def rails_image(h, w, seed, channel_tilt=True):
    """An RGB image of node_ref.rails_mask's horizontal wires: dark strokes on a light, slightly noisy page whose channels differ (so a
    wrong channel order changes grey values near the threshold's edge)."""
    rng = np.random.default_rng(seed)
    img = rng.integers(225, 256, size=(h, w, 3), dtype=np.uint8)
    if channel_tilt:
        img[..., 0] -= 40                                             # a reddish-poor page: R and B weights are not interchangeable
    img[R.rails_mask(h, w, seed) > 0] = (10, 20, 60)
    return img


def segments_image(h, w, seed, segments):
    """The same page with filled rectangles [x0, y0, x1, y1) as wires, dark unless three channel values follow the corners: a test can place
    every wire end where it wants it, and colour a wire so that only one channel order sees it."""
    rng = np.random.default_rng(seed)
    img = rng.integers(225, 256, size=(h, w, 3), dtype=np.uint8)
    img[..., 0] -= 40
    for seg in segments:
        x0, y0, x1, y1 = seg[:4]
        img[y0:y1, x0:x1] = tuple(seg[4:7]) if len(seg) > 4 else (10, 20, 60)
    return img


def golden_image(spec):
    if spec["gen"] == "rails":
        return rails_image(spec["h"], spec["w"], spec["seed"])
    if spec["gen"] == "segments":
        return segments_image(spec["h"], spec["w"], spec["seed"], spec["segments"])
    from synth import circuit_image
    return circuit_image(spec["h"], spec["w"], seed=spec["seed"])


def plane_checksum(m):
    """Position-sensitive checksum of a u8 plane."""
    v = m.astype(np.int64).ravel()
    return int(((v * (np.arange(v.size, dtype=np.int64) % 65521 + 1)).sum()) % (2 ** 61 - 1))


def mask_summary(m):
    return {"shape": list(m.shape), "sum": int(m.astype(np.int64).sum()), "checksum": plane_checksum(m)}
