"""Numpy / scipy restatement of the mask utilities of upstream's sam2/utils/amg.py that circuitvision_amd/amg_utils.py runs on the GPU
(csrc/mask_rle.hip, csrc/mask_cc.hip): mask_to_rle_pytorch, rle_to_mask, area_from_rle, remove_small_regions and
SAM2AutomaticMaskGenerator.postprocess_small_regions -- plus the seeded rows of tests/test_amg_post_gpu.py and the deliberately wrong
variants with which tests/test_amg_post_ref_cpu.py proves that the rows tell them apart.  TEST INFRASTRUCTURE ONLY; needs no GPU.

RLE: the plane in column-major order (y fastest); runs alternate and start with a run of zeros (0 when pixel (0, 0) is set); a run goes on
across a column end; the runs sum to H * W.
Removal, on u8 planes whose foreground is a non-zero byte, components 8-connected (scipy.ndimage.label with the 3 x 3 structure, as
tests/mask_cc_ref.py): holes -- every background component of area < min_area becomes 255; islands, on the result of the holes phase
labelled again -- every foreground component of area < min_area becomes 0, but where every one is that small the largest stays ([UP] the
raster-first one among equals: cv2's label order, cv2 is not available to confirm).  Other bytes keep their value.  `changed` = a pixel
was filled or removed.
Post-process: both phases per mask, boxes of the final planes (inclusive corners, {0, 0, 0, 0} for an empty plane), torchvision NMS with
score 1 for an unchanged mask and 0 for a changed one (ties to the lower index); survivors in NMS order; area and bbox of the final plane."""
import functools
import zlib

import numpy as np
import torch

from mask_cc_ref import EIGHT, FOUR, label_plane
from oracle.nms import torchvision_nms

RLE_MUTANTS = ("rle_row_major", "rle_no_leading_zero", "rle_break_at_column_end")
REMOVE_MUTANTS = ("single_pass", "holes_4_connected", "islands_4_connected", "le_instead_of_lt", "no_keep_largest", "keep_last_largest")
POST_MUTANTS = ("bbox_not_updated", "nms_prefers_changed", "order_not_unchanged_first")
PHASES = {1: "holes", 2: "islands", 3: "both"}
INFO = ("changed", "area", "x0", "y0", "x1", "y1", "filled", "removed")


# ---- RLE ------------------------------------------------------------------------------------------------------------------------------------------
def mask_to_rle(plane, mutant=None):
    """[H, W] (non-zero = set) -> {"size": [H, W], "counts": [...]}."""
    assert mutant in (None,) + RLE_MUTANTS, mutant
    m = np.asarray(plane) != 0
    H, W = m.shape
    if mutant == "rle_break_at_column_end":                                      # every column closes its run; a 0 keeps the alternation
        counts, value = [], False
        for x in range(W):
            for c, v in _runs(m[:, x]):
                if v != value:
                    counts.append(0)
                counts.append(c)
                value = not v
        if not counts:
            counts = [0]
        return {"size": [H, W], "counts": counts}
    flat = m.ravel() if mutant == "rle_row_major" else m.T.ravel()
    counts = []
    if flat[0] and mutant != "rle_no_leading_zero":
        counts.append(0)
    counts += [c for c, _ in _runs(flat)]
    return {"size": [H, W], "counts": counts}


def _runs(flat):
    """[(length, value)] of the maximal runs of a 1-D bool array."""
    edges = np.flatnonzero(flat[1:] != flat[:-1]) + 1
    bounds = np.concatenate([[0], edges, [flat.size]])
    return [(int(b - a), bool(flat[a])) for a, b in zip(bounds[:-1], bounds[1:])]


def rle_to_mask(rle):
    """upstream's rle_to_mask, loop and all -> bool [H, W]."""
    h, w = rle["size"]
    mask = np.empty(h * w, dtype=bool)
    idx, parity = 0, False
    for count in rle["counts"]:
        mask[idx:idx + count] = parity
        idx += count
        parity ^= True
    assert idx == h * w
    return mask.reshape(w, h).transpose()


def area_from_rle(rle):
    return sum(rle["counts"][1::2])


def stack_rle(planes):
    """u8 [N, H, W] -> (offsets int64 [N + 1], counts int64 [total]) as cvmi_mask_rle lays them out."""
    runs = [mask_to_rle(p)["counts"] for p in planes]
    return np.cumsum([0] + [len(r) for r in runs]), np.asarray([c for r in runs for c in r], dtype=np.int64)


# ---- small regions --------------------------------------------------------------------------------------------------------------------------------
def remove_small_regions(plane, min_area, mode, mutant=None):
    """u8 [H, W] -> (the new plane u8, info int64 [8])."""
    assert mode in ("holes", "islands", "both") and min_area > 0 and mutant in (None,) + REMOVE_MUTANTS, (mode, min_area, mutant)
    out = np.array(plane, dtype=np.uint8)
    small = (lambda a: a <= min_area) if mutant == "le_instead_of_lt" else (lambda a: a < min_area)
    filled = removed = 0
    if mutant == "single_pass" and mode == "both":
        # one labelling of the input serves both phases: the islands phase judges every foreground pixel of the filled plane by the area its
        # pixel had in the input -- a filled hole by its hole's -- and has no second labelling to find a largest component with
        area = label_plane(out == 0)[1] + label_plane(out != 0)[1]
        fill = (out == 0) & small(area)
        out[fill] = 255
        rem = (out != 0) & small(area)
        out[rem] = 0
        filled, removed = int(fill.sum()), int(rem.sum())
    else:
        if mode in ("holes", "both"):
            _, area = label_plane(out == 0, FOUR if mutant == "holes_4_connected" else EIGHT)
            fill = (out == 0) & small(area)
            out[fill] = 255
            filled = int(fill.sum())
        if mode in ("islands", "both"):
            fg = out != 0
            lab, area = label_plane(fg, FOUR if mutant == "islands_4_connected" else EIGHT)
            rem = fg & small(area)
            if rem.any() and not (fg & ~rem).any() and mutant != "no_keep_largest":          # every component is small: the largest stays
                labels = np.unique(lab[fg])                                      # label = 1 + the raster-first pixel: ascending = raster order
                sizes = np.array([area[lab == l][0] for l in labels])
                ties = labels[sizes == sizes.max()]
                rem &= lab != (ties[-1] if mutant == "keep_last_largest" else ties[0])
            out[rem] = 0
            removed = int(rem.sum())
    ys, xs = np.nonzero(out)
    box = [int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())] if ys.size else [0, 0, 0, 0]
    return out, np.array([int(filled + removed > 0), int(ys.size)] + box + [filled, removed], dtype=np.int64)


def remove_small_stack(planes, min_area, phases, mutant=None):
    """u8 [N, H, W], phases 1 / 2 / 3 -> (u8 [N, H, W], info int64 [N, 8])."""
    res = [remove_small_regions(p, min_area, PHASES[phases], mutant) for p in planes]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])


def postprocess_small_regions(dicts, min_area, nms_thresh, output_mode="binary_mask", mutant=None):
    """A list as generate() returns it (segmentation: u8 [H, W], any device) -> the post-processed list (segmentation: u8 CPU tensors, or RLE dicts)."""
    assert mutant in (None,) + POST_MUTANTS and output_mode in ("binary_mask", "uncompressed_rle"), (mutant, output_mode)
    if not dicts:
        return []
    planes = [torch.as_tensor(d["segmentation"]).cpu().numpy() for d in dicts]
    res = [remove_small_regions(p, min_area, "both") for p in planes]
    info = np.stack([r[1] for r in res])
    unchanged = (info[:, 0] == 0).astype(np.float32)
    scores = 1.0 - unchanged if mutant == "nms_prefers_changed" else unchanged
    keep = torchvision_nms(torch.as_tensor(info[:, 2:6], dtype=torch.float32), torch.as_tensor(scores), nms_thresh).tolist()
    if mutant == "order_not_unchanged_first":
        keep = sorted(keep)
    out = []
    for i in keep:
        _, area, x0, y0, x1, y1 = (int(v) for v in info[i, :6])
        d = dict(dicts[i])
        d["segmentation"] = mask_to_rle(res[i][0]) if output_mode == "uncompressed_rle" else torch.from_numpy(res[i][0])
        d["area"] = area
        d["bbox"] = list(dicts[i]["bbox"]) if mutant == "bbox_not_updated" else [x0, y0, x1 - x0, y1 - y0]
        out.append(d)
    return out


# ---- the rows of tests/test_amg_post_gpu.py -----------------------------------------------------------------------------------------------------------
def art(*rows):
    """'#' = 255, '1' = 1, anything else = 0 -> u8 [h, w]"""
    return np.array([[255 if c == "#" else 1 if c == "1" else 0 for c in row] for row in rows], dtype=np.uint8)


def _rng(rid, seed=0):
    return np.random.RandomState((zlib.crc32(("amg_post_" + rid).encode()) + seed) & 0x7FFFFFFF)


def _random(rid, N, H, W, density):
    return ((_rng(rid).rand(N, H, W) < density) * 255).astype(np.uint8)


def _checker(first):
    """An 8 x 8 checkerboard.  With an even height a column's last pixel equals the next column's first, so its runs join across every column end:
    57 runs starting clear, 58 starting set -- not one per pixel."""
    yy, xx = np.mgrid[0:8, 0:8]
    return (((yy + xx) % 2 == (0 if first else 1)) * 255).astype(np.uint8)[None]


def _alternating(first):
    """8 x 8 with every pixel its own run, H * W runs starting clear and H * W + 1 starting set: the values alternate in SCAN order (x * H + y),
    which at an even height is a pattern of rows, not a checkerboard."""
    yy, xx = np.mgrid[0:8, 0:8]
    return (((xx * 8 + yy) % 2 == (0 if first else 1)) * 255).astype(np.uint8)[None]


def _column_pairs():
    """plane 0: the last pixel of column 2 and the first of column 3 both set (one run across the column end); plane 1: the second one clear."""
    m = np.zeros((2, 5, 6), dtype=np.uint8)
    m[0, 4, 2] = m[0, 0, 3] = m[1, 4, 2] = 255
    return m


def _mixed_33():
    m = _random("planes_33", 33, 9, 9, 0.4)
    m[0] = m[7] = m[32] = 0
    m[1] = m[8] = 255
    return m


@functools.lru_cache(maxsize=None)
def rle_rows():
    """((id, u8 [N, H, W]), ...).  Once per process, never modified."""
    rows = [("clear_1x1", np.zeros((1, 1, 1), np.uint8)), ("set_1x1", np.full((1, 1, 1), 255, np.uint8)),
            ("row_1x7", art(".##.#.#")[None]), ("column_7x1", art(".##.#.#").T[None].copy()),
            ("known_2x2", np.stack([art(".#", "##"), art("#.", "..")])), ("all_set_5x3", np.full((1, 5, 3), 1, np.uint8)),
            ("checker_clear_first", _checker(False)), ("checker_set_first", _checker(True)),
            ("alternating_clear_first", _alternating(False)), ("alternating_set_first", _alternating(True))]
    for H, W in ((63, 65), (64, 64), (65, 63), (130, 70)):
        for density in (0.5, 0.02):
            rid = "random_%dx%d_d%g" % (H, W, density)
            rows.append((rid, _random(rid, 2, H, W, density)))
    rows += [("planes_1x300", _random("planes_1x300", 3, 1, 300, 0.3)), ("planes_300x1", _random("planes_300x1", 3, 300, 1, 0.3)),
             ("planes_33", _mixed_33()), ("column_pairs", _column_pairs())]
    for _, m in rows:
        m.setflags(write=False)
    return tuple(rows)


def _blobs(rid, N, H, W, seed=0):
    """Per plane: a filled ellipse that reaches over the 64-pixel seams, with pinholes of 1 .. 6 pixels in it and specks of 1 .. 6 pixels outside,
    two-pixel ones ACROSS each seam among them; plane 0 has neither (unchanged), the others both.  Even planes' foreground bytes are 1."""
    rng = _rng(rid, seed)
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.zeros((N, H, W), dtype=np.uint8)
    for n in range(N):
        cy, cx = H * (0.3 + 0.4 * rng.rand()), W * (0.3 + 0.4 * rng.rand())
        blob = ((yy - cy) / (0.42 * H)) ** 2 + ((xx - cx) / (0.42 * W)) ** 2 < 1
        out[n][blob] = 255 if n % 2 else 1
        if n == 0:                                                              # a plain rectangle: nothing small in either phase
            out[0] = 0
            out[0, H // 4:3 * H // 4, W // 4:3 * W // 4] = 1
            continue
        for _ in range(12):                                                      # short strokes: clear inside the blob, set outside
            y, x, dy, dx, k = rng.randint(H), rng.randint(W), rng.randint(-1, 2), rng.randint(-1, 2), rng.randint(1, 7)
            value = 0 if blob[y, x] else 255
            for s in range(k):
                py, px = y + s * dy, x + s * dx
                if 0 <= py < H and 0 <= px < W and blob[py, px] == blob[y, x]:
                    out[n, py, px] = value
        for y, x, dy, dx in [(rng.randint(H), 63, 0, 1) for _ in range(4) if W > 64] + [(63, rng.randint(W), 1, 0) for _ in range(4) if H > 64]:
            if blob[y, x] == blob[y + dy, x + dx]:                               # a pair across the seam, one pixel on each side
                out[n, y, x] = out[n, y + dy, x + dx] = 0 if blob[y, x] else 255
    return out


def _exact_areas():
    """min_area = 4: islands of 4 and 3 pixels beside a block with holes of 4 and 3 pixels."""
    return art("####........##",
               "............#.",
               ".###..........",
               "..............",
               ".############.",
               ".#....###...#.",
               ".############.",
               ".############.")[None]


def _diagonals():
    """plane 0: a foreground diagonal, one 8-connected component of 5 pixels.  plane 1: a pocket of 2 pixels joined to the outer background only
    through a diagonal gap -- not a hole of its own."""
    return np.stack([art("#.......", ".#......", "..#.....", "...#....", "....#...", "........", "........"),
                     art("........", ".####...", ".#..#...", ".###....", "........", "........", "........")])


def _all_small():
    """min_area = 5.  plane 0: components of 2, 3 and 1 pixels, the 3 stays.  plane 1: 3, 3 and 2, the raster-first 3 stays (the tie row)."""
    return np.stack([art("##.......", ".........", "...###...", ".........", "........#", "........."),
                     art(".........", ".###.....", ".........", ".....#...", ".....##..", "##.......")])


def _plain():
    """an empty plane, a full plane, and a plane whose foreground bytes are 1 with nothing small in it"""
    m = np.zeros((3, 20, 24), dtype=np.uint8)
    m[1] = 255
    m[2, 3:15, 4:20] = 1
    return m


def _spiral(n=130):
    """plane 0: a one-pixel-wide square spiral (arms one clear pixel apart) through every 64 x 64 tile of an n x n plane: one component, and the
    channel between its arms one background component.  plane 1: the same, cut on a straight arm about 30 pixels before its inner end: a short tail."""
    m = np.zeros((n, n), dtype=np.uint8)
    inside = lambda y, x: 0 <= y < n and 0 <= x < n
    y, x, dy, dx, path = 0, 0, 0, 1, [(0, 0)]
    m[0, 0] = 255
    while True:
        for _ in range(2):
            ny, nx, ay, ax = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            if inside(ny, nx) and not m[ny, nx] and not (inside(ay, ax) and m[ay, ax]):
                break
            dy, dx = dx, -dy                                                     # turn right
        else:
            break
        y, x = ny, nx
        m[y, x] = 255
        path.append((y, x))
    straight = lambda i: path[i - 2][0] == path[i + 2][0] or path[i - 2][1] == path[i + 2][1]
    two = np.stack([m, m])
    two[1][path[next(i for i in range(len(path) - 30, len(path) - 2) if straight(i))]] = 0
    return two


@functools.lru_cache(maxsize=None)
def remove_rows():
    """((id, u8 [N, H, W], min_area), ...).  Once per process, never modified."""
    rows = [("known_1x3", art("#.#")[None], 2), ("known_1x1", np.zeros((1, 1, 1), np.uint8), 2), ("exact_areas", _exact_areas(), 4),
            ("diagonals", _diagonals(), 3), ("all_small", _all_small(), 5), ("plain", _plain(), 6), ("spiral_130", _spiral(), 40)]
    for H, W in ((63, 65), (64, 64), (65, 63), (130, 70)):
        rid = "blobs_%dx%d" % (H, W)
        rows.append((rid, _blobs(rid, 3, H, W), 5))
    rows.append(("blobs_33_planes", _blobs("blobs_33_planes", 33, 40, 72), 5))
    for _, m, _a in rows:
        m.setflags(write=False)
    return tuple(rows)


SEEDED_REMOVE_ROWS = ("blobs_63x65", "blobs_64x64", "blobs_65x63", "blobs_130x70", "blobs_33_planes")


def _dict(plane, score, index):
    ys, xs = np.nonzero(plane)
    x0, y0, x1, y1 = int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())
    H, W = plane.shape
    return {"segmentation": torch.from_numpy(np.ascontiguousarray(plane)), "area": int(ys.size), "bbox": [x0, y0, x1 - x0, y1 - y0], "predicted_iou": score,
            "point_coords": [[float(index), 0.5]], "stability_score": 0.96 + index / 256, "crop_box": [0, 0, W, H]}


@functools.lru_cache(maxsize=None)
def post_case():
    """(dicts, min_area, nms_thresh): A with a speck outside its box (index 0), B with a speck (index 1), B clean (index 2), C clean far away
    (index 3).  -> NMS order: 2, 3 (unchanged), then 0 (changed); 1 is suppressed by 2, whose plane it equals after the removal."""
    H, W = 40, 70
    a, b, c = (np.zeros((H, W), dtype=np.uint8) for _ in range(3))
    a[5:15, 5:20] = 255
    b[20:35, 30:50] = 255
    c[2:12, 55:68] = 255
    a_speck, b_speck = a.copy(), b.copy()
    a_speck[30, 3] = 255                                                         # outside A's box: the removal shrinks bbox
    b_speck[37:39, 60] = 255
    return tuple(_dict(p, s, i) for i, (p, s) in enumerate(((a_speck, 0.9), (b_speck, 0.95), (b, 0.85), (c, 0.8)))), 4, 0.7
