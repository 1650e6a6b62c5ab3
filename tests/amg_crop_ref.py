"""Plain reference of the automatic mask generator's crop layers (circuitvision_amd/amg.py with crop_n_layers > 0, amg_utils.generate_crop_boxes,
csrc/mask_amg.hip: cvmi_amg_select_crop, cvmi_amg_score_window): upstream's crop boxes and layer grids, is_box_near_crop_edge, the uncrop of
boxes, points and masks (zero padding), the per-crop pipeline on tests/amg_ref.py's score_planes / select / nms, the NMS across the crops
(score 1 / crop area, ties to the lower index) and the output dicts -- on the CPU, written independently of the package --, plus the rows of
the GPU tests (tests/test_amg_crop_gpu.py) and the deliberately wrong variants (CROP_MUTANTS) with which tests/test_amg_crop_ref_cpu.py proves
that those rows tell them apart.  Importing this module needs neither a GPU nor the library."""
import math

import numpy as np
import torch

import amg_ref

CROP_MUTANTS = ("tol_lt", "box_max_exclusive", "image_edge_not_exempt", "crop_order_yx", "overlap_ceil", "grid_not_downscaled", "cross_nms_by_iou",
                "prefer_larger_crop", "points_not_uncropped", "crop_box_xyxy", "window_off_by_one")
RATIO = 512 / 1500
EDGE_TOL = 20


# ---- geometry ---------------------------------------------------------------------------------------------------------------------------------------
def crop_boxes(H, W, n_layers, ratio=RATIO, mutant=None):
    """-> (boxes [x0, y0, x1, y1] with exclusive ends, layer of each).  Box 0 is the image; layer i + 1 has n = 2 ** (i + 1) crops per side."""
    assert mutant in (None,) + CROP_MUTANTS, mutant
    boxes, layers = [[0, 0, W, H]], [0]
    for i in range(n_layers):
        n = 2 ** (i + 1)
        raw = ratio * min(H, W) * (2 / n)
        overlap = math.ceil(raw) if mutant == "overlap_ceil" else int(raw)
        cw, ch = math.ceil((overlap * (n - 1) + W) / n), math.ceil((overlap * (n - 1) + H) / n)
        xs, ys = [int((cw - overlap) * k) for k in range(n)], [int((ch - overlap) * k) for k in range(n)]
        pairs = [(x, y) for y in ys for x in xs] if mutant == "crop_order_yx" else [(x, y) for x in xs for y in ys]
        for x, y in pairs:
            boxes.append([x, y, min(x + cw, W), min(y + ch, H)])
            layers.append(i + 1)
    return boxes, layers


def layer_grids(n_per_side, n_layers, scale, mutant=None):
    """One grid per layer: layer i has int(n_per_side / scale ** i) points per side."""
    return [amg_ref.point_grid(n_per_side if mutant == "grid_not_downscaled" else int(n_per_side / scale ** i)) for i in range(n_layers + 1)]


# ---- the border filter ---------------------------------------------------------------------------------------------------------------------------------
def near_crop_edge(boxes, crop, H, W, tol=EDGE_TOL, mutant=None):
    """upstream's is_box_near_crop_edge: boxes int [n, 4] in CROP coordinates (inclusive maxima, the empty mask's zeros as they are), crop
    [x0, y0, x1, y1] -> bool [n]: some side within tol of the crop's side and not within tol of the image's."""
    b = np.asarray(boxes, dtype=np.int64).reshape(-1, 4).copy()
    if mutant == "box_max_exclusive":
        b[:, 2:] += 1
    b += np.array([crop[0], crop[1], crop[0], crop[1]])
    close = (lambda d: d < tol) if mutant == "tol_lt" else (lambda d: d <= tol)
    near_crop = close(np.abs(b - np.asarray(crop)[None]))
    near_image = close(np.abs(b - np.array([0, 0, W, H])[None]))
    if mutant == "image_edge_not_exempt":
        near_image[:] = False
    return (near_crop & ~near_image).any(1)


def select(stats, iou, n_valid, pred_iou_thresh, stability_score_thresh, crop, H, W, tol=EDGE_TOL, mutant=None):
    """amg_ref.select and the border filter: the kept planes' indices, in candidate order."""
    kept = amg_ref.select(stats, iou, n_valid, pred_iou_thresh, stability_score_thresh)
    cut = near_crop_edge(np.asarray(stats)[:, 3:7], crop, H, W, tol, mutant)
    return np.array([i for i in kept if not cut[i]], dtype=np.int64)


# ---- uncrop ----------------------------------------------------------------------------------------------------------------------------------------------
def uncrop_mask(mask, crop, H, W, mutant=None):
    """u8 [ch, cw] -> u8 [H, W]: the mask at the crop's origin, zeros around it."""
    x0, y0 = crop[0], crop[1]
    ch, cw = mask.shape
    out = torch.zeros(H, W, dtype=mask.dtype)
    out[y0:y0 + ch, x0:x0 + cw] = mask
    return torch.roll(out, 1, dims=1) if mutant == "window_off_by_one" else out


# ---- the pipeline ----------------------------------------------------------------------------------------------------------------------------------------
def generate_crops_ref(crops, H, W, pred_iou_thresh, stability_score_thresh, lv, box_nms_thresh, crop_nms_thresh, mutant=None, info=None):
    """One image.  crops: per crop, in crop order, dict(box=[x0, y0, x1, y1], iou=f32 [Np, C], maps=f32 [Np * C, ch, cw] (the decoder's
    planes resized to the crop), grid=float64 [n, 2], n_points=n[, stats=amg_ref.score_planes(maps, *lv), computed once by a caller that runs this
    several times]) -- planes of points >= n_points are padding.  -> the output dicts, in the
    order of the NMS across the crops.  info (a dict) receives per-crop counts: passed the score filters, cut by the border filter, suppressed by
    the per-crop NMS, and after the merge `cross_suppressed` and `crops_in_result`."""
    assert mutant in (None,) + CROP_MUTANTS, mutant
    lo, mid, hi = lv
    surv = []                                                                    # (crop index, plane index, stats row, iou, stability)
    counts = []
    for c, crop in enumerate(crops):
        x0, y0, x1, y1 = crop["box"]
        C = crop["iou"].shape[1]
        assert tuple(crop["maps"].shape[1:]) == (y1 - y0, x1 - x0)
        stats = crop["stats"] if "stats" in crop else amg_ref.score_planes(crop["maps"], lo, mid, hi)
        iou = np.asarray(crop["iou"], dtype=np.float32).reshape(-1)
        stab = amg_ref.stability(stats)
        passed = amg_ref.select(stats, iou, crop["n_points"] * C, pred_iou_thresh, stability_score_thresh)
        kept = select(stats, iou, crop["n_points"] * C, pred_iou_thresh, stability_score_thresh, crop["box"], H, W, EDGE_TOL, mutant)
        order = amg_ref.nms(stats[kept, 3:7], iou[kept], box_nms_thresh)
        counts.append(dict(passed=len(passed), cut=len(passed) - len(kept), suppressed=len(kept) - len(order)))
        surv += [(c, int(kept[p]), stats[int(kept[p])], float(iou[int(kept[p])]), float(stab[int(kept[p])])) for p in order]
    keep = list(range(len(surv)))
    if len(crops) > 1 and surv:
        boxes = [[int(s[3]) + crops[c]["box"][0], int(s[4]) + crops[c]["box"][1], int(s[5]) + crops[c]["box"][0], int(s[6]) + crops[c]["box"][1]]
                 for c, _, s, _, _ in surv]
        area = np.array([(crops[c]["box"][2] - crops[c]["box"][0]) * (crops[c]["box"][3] - crops[c]["box"][1]) for c, *_ in surv], dtype=np.float32)
        scores = np.float32(1.0) / area
        if mutant == "prefer_larger_crop":
            scores = area
        if mutant == "cross_nms_by_iou":
            scores = np.array([s[3] for s in surv], dtype=np.float32)
        keep = amg_ref.nms(boxes, scores, crop_nms_thresh).tolist()
    out = []
    for p in keep:
        c, i, s, iou_i, stab_i = surv[p]
        crop = crops[c]
        cx0, cy0, cx1, cy1 = crop["box"]
        cw, ch = cx1 - cx0, cy1 - cy0
        bx0, by0, bx1, by1 = (int(v) for v in s[3:7])
        C = crop["iou"].shape[1]
        gx, gy = crop["grid"][i // C]
        point = [float(gx * cw), float(gy * ch)] if mutant == "points_not_uncropped" else [float(gx * cw + cx0), float(gy * ch + cy0)]
        mask = (crop["maps"][i] > mid).to(torch.uint8) * 255
        out.append({"segmentation": uncrop_mask(mask, crop["box"], H, W, mutant), "area": int(s[2]), "bbox": [bx0 + cx0, by0 + cy0, bx1 - bx0, by1 - by0],
                    "predicted_iou": iou_i, "point_coords": [point], "stability_score": stab_i,
                    "crop_box": [cx0, cy0, cx1, cy1] if mutant == "crop_box_xyxy" else [cx0, cy0, cw, ch]})
    if info is not None:
        info.update(per_crop=counts, cross_suppressed=len(surv) - len(keep), crops_in_result=sorted({surv[p][0] for p in keep}))
    return out


# ---- the rows of the GPU tests -----------------------------------------------------------------------------------------------------------------------------
# The border filter: (crop [x0, y0, x1, y1], (W, H) of the image, [(label, box in crop coordinates, expected kept)]).  Every row passes the score
# filters.  The issue's two crops have their right and bottom sides ON the image's, so the right / bottom cases use the crops at the origin.
BORDER_CASES = (
    ([64, 32, 160, 96], (160, 96), [
        ("left_20", (20, 30, 60, 40), False), ("left_21", (21, 30, 60, 40), True),
        ("top_20", (30, 20, 60, 40), False), ("dropped_between_kept", (5, 30, 60, 40), False), ("top_21", (30, 21, 60, 40), True),
        ("right_on_image_edge", (30, 30, 95, 40), True), ("bottom_on_image_edge", (30, 30, 60, 63), True),
        ("empty_in_interior_crop", (0, 0, 0, 0), False), ("clear", (40, 25, 50, 35), True)]),
    ([85, 85, 256, 256], (256, 256), [
        ("left_20", (20, 40, 100, 100), False), ("left_21", (21, 40, 100, 100), True), ("top_20", (40, 20, 100, 100), False),
        ("top_21", (40, 21, 100, 100), True), ("both_edges", (40, 40, 170, 170), True), ("empty_in_interior_crop", (0, 0, 0, 0), False)]),
    ([0, 0, 96, 64], (160, 96), [
        ("right_20", (30, 30, 76, 40), False), ("right_21", (30, 30, 75, 40), True), ("bottom_20", (30, 10, 60, 44), False),
        ("bottom_21", (30, 10, 60, 43), True), ("empty_at_the_origin", (0, 0, 0, 0), True), ("left_on_image_edge", (0, 0, 50, 30), True)]),
    ([0, 0, 172, 172], (256, 256), [
        ("right_20", (30, 30, 152, 100), False), ("right_21", (30, 30, 151, 100), True), ("bottom_20", (30, 30, 100, 152), False),
        ("bottom_21", (30, 30, 100, 151), True)]),
)

# The window writer: (id, M, h, w, H, W, PH, PW, wx0, wy0) -- M source planes h x w resized to an H x W window at (wx0, wy0) of a PH x PW plane.
WINDOW_ROWS = tuple(("w33x45_in_64x64_x%d_y%d" % (x, y), 2, 16, 16, 33, 45, 64, 64, x, y) for y in (0, 31) for x in (0, 1, 2, 3, 19)) + (
    ("pw63_bytes_odd_stride", 3, 16, 16, 33, 45, 35, 63, 5, 1),
    ("pw66_bytes", 3, 16, 16, 33, 45, 35, 66, 7, 2),
    ("one_pixel_plane", 1, 8, 8, 1, 1, 1, 1, 0, 0),
    ("one_pixel_in_5x7", 2, 8, 8, 1, 1, 5, 7, 3, 2),
    ("window_is_plane_64x64", 3, 16, 16, 64, 64, 64, 64, 0, 0),
    ("window_is_plane_67x131", 5, 16, 12, 67, 131, 67, 131, 0, 0),
    ("past_one_chunk_1x1028", 2, 1, 8, 1, 4, 1, 1028, 1024, 0),
    ("tall_two_bands", 2, 16, 16, 40, 20, 90, 24, 3, 45),
)


def grid_cap_window_row(grid_cap, chunk):
    """More units than the scorer's capped grid: one plane row of grid_cap + 1 chunks of columns, the window across the last chunk boundary."""
    return ("grid_cap_plus_1", 2, 1, 64, 1, 2053, 1, grid_cap * chunk + 8, grid_cap * chunk - 2049, 0)


def window_planes(row):
    """f32 [M, h, w] random source planes of a window row (values anywhere: no precondition)."""
    g = torch.Generator().manual_seed(977 + sum(int(v) for v in row[1:]))
    return torch.randn(row[1], row[2], row[3], generator=g) * 1.5


# ---- a synthetic image for the merge (no model): what test_amg_crop_ref_cpu.py runs the mutants on ---------------------------------------------------------
def merge_case():
    """A 256 x 256 image, one crop layer (boxes 1 and 2 have areas 172 x 172 and 172 x 171), a 2 x 2 grid of single-candidate points whose
    maps are rectangles: -> (crops, H, W, thresholds...).  The rectangles are chosen so that the border filter cuts some, the per-crop NMS and
    the NMS across the crops each suppress some, and the result holds masks of the image and of several layer-1 crops."""
    H = W = 256
    boxes, _ = crop_boxes(H, W, 1)
    grid = amg_ref.point_grid(2)
    rects = {                                                                    # per crop: (x0, y0, x1, y1 inclusive, in crop coordinates; predicted IoU)
        0: [((30, 30, 90, 90), 0.9), ((31, 31, 90, 90), 0.85), ((150, 150, 220, 220), 0.8), ((100, 10, 140, 40), 0.7)],
        1: [((30, 30, 90, 90), 0.95), ((100, 10, 140, 40), 0.6), ((60, 60, 160, 120), 0.9), ((25, 120, 60, 145), 0.9)],
        2: [((30, 30, 90, 100), 0.9), ((30, 25, 90, 100), 0.8), ((10, 60, 30, 90), 0.9), ((40, 110, 60, 170), 0.9)],
        3: [((70, 70, 130, 130), 0.9), ((30, 30, 60, 60), 0.9), ((10, 100, 60, 140), 0.9), ((100, 100, 170, 135), 0.9)],
        4: [((65, 65, 100, 135), 0.9), ((25, 25, 60, 60), 0.9), ((30, 90, 60, 120), 0.75), ((100, 25, 160, 60), 0.9)],
    }
    crops = []
    for c, box in enumerate(boxes):
        cw, ch = box[2] - box[0], box[3] - box[1]
        maps = torch.full((4, ch, cw), -5.0)
        for i, ((x0, y0, x1, y1), _) in enumerate(rects[c]):
            maps[i, y0:y1 + 1, x0:x1 + 1] = 5.0
        crops.append(dict(box=box, iou=np.array([[s] for _, s in rects[c]], dtype=np.float32), maps=maps, grid=grid, n_points=4))
    return crops, H, W, dict(pred_iou_thresh=0.5, stability_score_thresh=0.9, lv=amg_ref.levels(0.0, 1.0), box_nms_thresh=0.7, crop_nms_thresh=0.7)
