"""Plain reference of the automatic mask generator (circuitvision_amd/amg.py, csrc/mask_amg.hip): upstream's SAM2AutomaticMaskGenerator at its
defaults (crop_n_layers = 0, use_m2m = False, min_mask_region_area = 0, multimask_output = True) restated in torch and numpy on the CPU --
the point grid, the per-plane scores of a resized logit map, the keep rule, box NMS (oracle.nms.torchvision_nms) and the output dicts --
plus the seeded rows of the scorer's GPU test and the deliberately wrong variants (AMG_MUTANTS) with which tests/test_amg_ref_cpu.py proves
that its cases tell them apart.  Importing this module needs neither a GPU nor the library.

Per plane, with the levels lo = thr - off, mid = thr, hi = thr + off:  n_hi = #(v > hi), n_lo = #(v > lo), area = #(v > mid), box = the
inclusive {min x, min y, max x, max y} of v > mid or {0, 0, 0, 0} for an empty mask (upstream's batched_mask_to_box), stability =
float32(n_hi) / float32(n_lo) (0 / 0 = NaN).  Keep iff iou > pred_iou_thresh and stability >= stability_score_thresh, among the first
n_valid planes only.  NMS on the float boxes, score = predicted IoU (stable descending sort: ties to the lower index), suppress on IoU >
box_nms_thresh with box area (x1 - x0) (y1 - y0); a NaN IoU does not suppress."""
import functools
import zlib

import numpy as np
import torch

from oracle.nms import torchvision_nms

AMG_MUTANTS = ("offset_sign", "hi_ge", "mid_ge", "lo_ge", "box_exclusive_max", "empty_box_whm1", "bbox_w_plus_1", "nms_by_index", "padding_selected",
               "area_of_lo")
KEYS = ("segmentation", "area", "bbox", "predicted_iou", "point_coords", "stability_score", "crop_box")


def levels(mask_threshold, offset):
    """(lo, mid, hi): computed in double, rounded once to f32 (returned as Python floats holding f32 values)."""
    return tuple(float(np.float32(v)) for v in (mask_threshold - offset, mask_threshold, mask_threshold + offset))


def point_grid(n):
    """upstream's build_point_grid: float64 [n * n, 2] (x, y) in [0, 1]^2, x fastest; offset 1 / (2 n), linspace(offset, 1 - offset, n)."""
    offset = 1.0 / (2 * n)
    side = np.linspace(offset, 1.0 - offset, n)
    return np.array([[x, y] for y in side for x in side], dtype=np.float64).reshape(n * n, 2)


def score_planes(maps, lo, mid, hi, mutant=None):
    """maps [M, H, W] (any float type) -> int64 [M, 8] = {n_hi, n_lo, area, x0, y0, x1, y1, 0}."""
    assert mutant in (None,) + AMG_MUTANTS, mutant
    if mutant == "offset_sign":
        lo, hi = hi, lo
    gt = lambda v, level, ge: (v >= level) if ge else (v > level)
    M, H, W = maps.shape
    out = torch.zeros(M, 8, dtype=torch.int64)
    for m in range(M):
        v = maps[m]
        on = gt(v, mid, mutant == "mid_ge")
        out[m, 0] = int(gt(v, hi, mutant == "hi_ge").sum())
        out[m, 1] = int(gt(v, lo, mutant == "lo_ge").sum())
        out[m, 2] = out[m, 1] if mutant == "area_of_lo" else int(on.sum())
        ys, xs = torch.nonzero(on, as_tuple=True)
        if ys.numel():
            e = 1 if mutant == "box_exclusive_max" else 0
            out[m, 3:7] = torch.tensor([int(xs.min()), int(ys.min()), int(xs.max()) + e, int(ys.max()) + e])
        elif mutant == "empty_box_whm1":
            out[m, 3:7] = torch.tensor([W, H, -1, -1])
    return out


def stability(stats):
    """f32 [M]: float32(n_hi) / float32(n_lo); 0 / 0 is NaN."""
    s = np.asarray(stats)
    with np.errstate(divide="ignore", invalid="ignore"):
        return s[:, 0].astype(np.float32) / s[:, 1].astype(np.float32)


def select(stats, iou, n_valid, pred_iou_thresh, stability_score_thresh, mutant=None):
    """Indices of the kept planes, in candidate order.  iou f32 [M]; the thresholds are compared as f32."""
    stab = stability(stats)
    iou = np.asarray(iou, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        keep = (iou > np.float32(pred_iou_thresh)) & (stab >= np.float32(stability_score_thresh))
    if mutant != "padding_selected":
        keep[n_valid:] = False
    return np.nonzero(keep)[0]


def nms(boxes, scores, thresh, mutant=None):
    """Kept positions in NMS order.  boxes [n, 4] inclusive integer corners (taken as floats), scores f32 [n]."""
    boxes = torch.as_tensor(np.asarray(boxes), dtype=torch.float32).reshape(-1, 4)
    scores = torch.as_tensor(np.asarray(scores), dtype=torch.float32).reshape(-1)
    if mutant == "nms_by_index":
        scores = -torch.arange(scores.numel(), dtype=torch.float32)
    return torchvision_nms(boxes, scores, thresh).numpy()


def generate_ref(low3, iou3, maps, grid, n_points, H, W, pred_iou_thresh, stability_score_thresh, lv, box_nms_thresh, mutant=None):
    """One image.  low3 [Np, C, h, w] (the decoder's planes; only their count enters), iou3 f32 [Np, C], maps f32 [Np * C, H, W] (the planes
    resized to the image), grid float64 [>= n_points, 2]; planes of points >= n_points are padding.  lv = levels(...).  -> the output dicts."""
    Np, C = iou3.shape[:2]
    assert low3 is None or tuple(low3.shape[:2]) == (Np, C)
    assert tuple(maps.shape) == (Np * C, H, W)
    lo, mid, hi = lv
    stats = score_planes(maps, lo, mid, hi, mutant)
    iou = np.asarray(iou3, dtype=np.float32).reshape(-1)
    kept = select(stats, iou, n_points * C, pred_iou_thresh, stability_score_thresh, mutant)
    stab = stability(stats)
    order = nms(stats[kept, 3:7], iou[kept], box_nms_thresh, mutant)
    out = []
    for pos in order:
        i = int(kept[pos])
        x0, y0, x1, y1 = (int(v) for v in stats[i, 3:7])
        gx, gy = grid[min(i // C, len(grid) - 1)]
        on = (maps[i] >= mid) if mutant == "mid_ge" else (maps[i] > mid)
        out.append({"segmentation": on.to(torch.uint8) * 255, "area": int(stats[i, 2]),
                    "bbox": [x0, y0, x1 - x0 + (1 if mutant == "bbox_w_plus_1" else 0), y1 - y0],
                    "predicted_iou": float(iou[i]), "point_coords": [[float(gx * W), float(gy * H)]], "stability_score": float(stab[i]),
                    "crop_box": [0, 0, W, H]})
    return out


def same_dicts(a, b):
    """Two output lists agree key for key and bit for bit (masks included; NaN equals NaN)."""
    if len(a) != len(b):
        return False
    for da, db in zip(a, b):
        if tuple(da) != KEYS or tuple(db) != KEYS:
            return False
        for k in KEYS:
            va, vb = da[k], db[k]
            if k == "segmentation":
                va, vb = torch.as_tensor(va).cpu(), torch.as_tensor(vb).cpu()
                if va.dtype != vb.dtype or va.shape != vb.shape or not torch.equal(va, vb):
                    return False
            elif isinstance(va, float):
                if type(vb) is not float or np.float64(va).tobytes() != np.float64(vb).tobytes() and not (va != va and vb != vb):
                    return False
            elif va != vb or type(va) is not type(vb):
                return False
    return True


# ---- the scorer's rows (tests/test_amg_gpu.py) -----------------------------------------------------------------------------------------------
# Level pairs (mask_threshold, stability_score_offset): the defaults' shape (three distinct levels) and a collapsed one (all three equal).
LEVEL_PAIRS = ((0.0, 1.0), (0.5, 0.0))
# (id, M, h, w, H, W, kind, seed).  kind "blob": a blob on a negative noisy background, every second plane with a second blob so that the
# boxes differ; "edge" / "flat": resample_ref.mask_operands of the named mask-return row (the blob wrapped round every border; an all-below and
# an all-above plane).  seed: moved until the fp64 reference is clear of all three levels of both pairs on EVERY pixel
# (test_amg_ref_cpu.py asserts it), so that a correct kernel cannot land on the other side of a level.
SCORER_ROWS = (
    ("one_pixel", 1, 8, 8, 1, 1, "blob", 0),
    ("up_13x29", 3, 8, 8, 13, 29, "blob", 0),
    ("exact_4x", 3, 16, 16, 64, 64, "blob", 0),
    ("up_67x131", 5, 16, 12, 67, 131, "blob", 1),
    ("down_9x7", 2, 16, 16, 9, 7, "blob", 0),
    ("planes_193", 193, 8, 8, 16, 16, "blob", 2),
    ("flat", 2, 6, 5, 13, 11, "mask_empty_and_full", 0),
    ("edge", 5, 12, 10, 37, 45, "mask_rects_dev_clip", 0),
)


def grid_cap_row(grid_cap, chunk):
    """The row one pixel past a single pass of the scorer's capped grid: one output row of grid_cap chunks of columns, plus one column."""
    return ("grid_cap_plus_1", 2, 1, 4096, 1, grid_cap * chunk + 1, "blob", 0)


@functools.lru_cache(maxsize=None)
def scorer_planes(row):
    """f32 [M, h, w] source planes of a row.  Once per process, never modified."""
    rid, M, h, w, H, W, kind, seed = row
    if kind != "blob":
        from resample_ref import mask_operands
        low = mask_operands(kind)
        assert tuple(low.shape) == (M, h, w), (rid, tuple(low.shape))
        return low
    g = torch.Generator().manual_seed(zlib.crc32(("amg_" + rid).encode()) + seed)
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    low = torch.randn(M, h, w, generator=g) * 2
    for m in range(M):
        cy, cx = h * (0.2 + 0.6 * ((m * 7) % 10) / 10), w * (0.75 - 0.5 * ((m * 3) % 10) / 10)
        blob = ((yy - cy) / (0.22 * h)) ** 2 + ((xx - cx) / (0.3 * w)) ** 2 < 1
        if m % 2:
            blob |= ((yy - (h - 1 - cy)) / (0.15 * h)) ** 2 + ((xx - (w - 1 - cx)) / (0.15 * w)) ** 2 < 1
        low[m] += torch.where(blob, 10.0, -10.0)
    return low


@functools.lru_cache(maxsize=None)
def scorer_reference(row):
    """The fp64 resize [M, H, W] of a row's planes (resample_ref.bil_explicit).  Once per process, never modified."""
    from resample_ref import bil_explicit
    return bil_explicit(scorer_planes(row), row[4], row[5])


def scorer_clear(row):
    """The precondition: the fp64 reference is clear of every level of every pair by resample_ref.clear_of's bound, on every pixel."""
    from resample_ref import clear_of
    ref = scorer_reference(row)
    return all(clear_of(ref, level) for pair in LEVEL_PAIRS for level in levels(*pair))
