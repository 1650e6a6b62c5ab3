"""Plain references of the resampling kernels in resample.hip -- the antialiased input transform (cvmi_sam2_transform and its batch / rects /
rects_dev / srcs forms) and the bilinear mask return (cvmi_bilinear_f32, cvmi_mask_postprocess and its sizes / rects_dev forms,
cvmi_mask_extent) -- the seeded operands of every row of op_matrix.RESAMPLE_ROWS and the bounds the resampling matrix
(tests/test_resample_matrix_gpu.py) holds the kernels to.  CPU only, numpy and plain torch: importing this module needs neither a GPU nor the
library.

The transform is stated from the formula of torch's _upsample_bilinear2d_aa, not through the kernel: per axis scale = in / out,
support = max(scale, 1), center = scale * (i + 0.5), taps from (int)(center - support + 0.5) to (int)(center + support + 0.5) clamped to the
source (the window, for a windowed form), triangle weights 1 - |tap + 0.5 - center| / support, normalised.  dtype = float64 is the yardstick
(tests/test_resample_ref_cpu.py cross-checks it against F.interpolate(double, antialias=True)); dtype = float32 ("chain32") is the same statement
with taps chosen and weights normalised in fp32 and the taps summed columns then rows, one after the other, as a plain fp32 implementation does.
The mask return's yardstick is helper_ref.bilinear_ref + mask_and_extent.  mutant= selects one deliberately wrong statement, so that the CPU
test can prove without a GPU that rows and bounds catch it.

`PYTHONPATH=. python tests/resample_ref.py` (from the repository root) prints the measured chain32 deviations behind CHAIN32_DEV."""
import functools
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from helper_ref import FACTOR, RTOL, bilinear_ref, mask_and_extent, rT
from helper_ref import operands as helper_operands

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
AA_MUTANTS = ("aa_taps_capped_16", "aa_no_antialias", "aa_center_no_half", "aa_window_reads_image", "aa_swap_moves_mean_std", "aa_second_window_table_restarts")
BIL_MUTANTS = ("bil_align_corners", "bil_no_low_clamp", "bil_extent_exclusive_max")
CLIP_MUTANTS = ("clip_moves_window",)
RESAMPLE_MUTANTS = AA_MUTANTS + BIL_MUTANTS + CLIP_MUTANTS

# |y - ref64| <= ATOL[family] + RTOL[stored type] |ref64| per element (helper_ref.RTOL: one step of the stored output).  ATOL = FACTOR x the largest
# |chain32 - ref64| over the rows of the family, measured on the CPU on the f32 outputs (main() below; the CPU test fails when a row change moves a
# measurement past its constant or leaves the constant more than 4 x too loose).  The factor covers what chain32 does not reproduce: fused
# multiply-adds and the kernels' reciprocal.  No kernel enters these numbers.
# measured largest |chain32 - ref64| per family (PYTHONPATH=. python tests/resample_ref.py), rounded up to two digits:
#   aa_transform   8.2e-6   the R = 1025 row from 40 x 24: 40 / 1025 is inexact in fp32, a tap centre near 40 is off by ~2e-6 source pixels, neighbouring
#                           noise pixels differ by up to 1 and (x - mean) / std divides by ~0.225.  The R = 16 rows (exact scales) measure 1.1e-6 at most
#   bilinear_edge  5.2e-5   (constant 5.8e-5: F.interpolate in fp32 may contract differently by host) fp32 source coordinates (64 -> 513: one ulp of 64
#                           is 7.6e-6) times the steepest slope of the blob input (~25 per source pixel), as helper_ref's `bilinear`
CHAIN32_DEV = {"aa_transform": 8.2e-6, "bilinear_edge": 5.8e-5}
ATOL = {k: FACTOR * v for k, v in CHAIN32_DEV.items()}


def tol_ratio(y, ref64, fam, stored):
    """max over elements of |y - ref64| / (ATOL[fam] + RTOL[stored] |ref64|): <= 1 passes.  Also returns the largest |y - ref64|."""
    err = (y.double() - ref64.double()).abs()
    if err.numel() == 0:
        return 0.0, 0.0
    return float((err / (ATOL[fam] + RTOL[stored] * ref64.double().abs())).max()), float(err.max())


def clear_of(ref, level, fam="bilinear_edge", stored="f32"):
    """No element of ref lies within the family's bound of `level`: a correct kernel cannot land on the other side."""
    return bool(((ref - level).abs() > ATOL[fam] + RTOL[stored] * ref.abs()).all())


def _gen(rid, seed=0):
    return torch.Generator().manual_seed(zlib.crc32(rid.encode()) + seed)


# ---- what the two device-table kernels promise (the comments above sam2_transform_rects_dev_kernel and rect_plane_size) --------------------------
def clip_window(rc, H, W, mutant=None):
    """{x0, y0, w, h} clipped to the H x W image: x0 into [0, W - 1], y0 into [0, H - 1], then w into [1, W - x0] and h into [1, H - y0]."""
    assert mutant in (None,) + CLIP_MUTANTS, mutant
    x0, y0, w, h = rc
    if mutant == "clip_moves_window":                       # an over-wide window keeps its size and is shifted back into the image
        w, h = min(max(w, 1), W), min(max(h, 1), H)
        return (min(max(x0, 0), W - w), min(max(y0, 0), H - h), w, h)
    x0, y0 = min(max(x0, 0), W - 1), min(max(y0, 0), H - 1)
    return (x0, y0, min(max(w, 1), W - x0), min(max(h, 1), H - y0))


def clip_plane(rc, plane_stride):
    """(H, W) of the plane a window {x0, y0, w, h} returns to under a fixed plane stride: both at least 1, W clamped to the stride, then H to stride // W."""
    W, H = max(rc[2], 1), max(rc[3], 1)
    W = min(W, plane_stride)
    return (min(H, plane_stride // W), W)


# ---- the antialiased transform ----------------------------------------------------------------------------------------------------------------------
def aa_axis(n_in, n_out, ft=np.float64, mutant=None, lo=0, hi=None):
    """(first tap [n_out], taps [n_out], weights [n_out, T]) of one axis, every operation in the numpy float type ft.  lo, hi: the tap range is
    clamped to [lo, hi) (mutants only: the default is the source itself)."""
    hi = n_in if hi is None else hi
    one, half = ft(1), ft(0.5)
    scale = ft(n_in) / ft(n_out)
    down = bool(scale >= one) and mutant != "aa_no_antialias"
    support = scale if down else one
    invscale = one / scale if down else one
    i = np.arange(n_out).astype(ft)
    center = scale * (i if mutant == "aa_center_no_half" else i + half)
    xmin = np.maximum(np.trunc(center - support + half).astype(np.int64), lo)
    xsize = np.minimum(np.trunc(center + support + half).astype(np.int64), hi) - xmin
    if mutant == "aa_taps_capped_16":
        xsize = np.minimum(xsize, 16)
    T = max(int(xsize.max()), 1)
    wt, total = np.zeros((n_out, T), ft), np.zeros(n_out, ft)
    for j in range(T):
        t = np.abs(((xmin + j).astype(ft) - center + half) * invscale)
        wt[:, j] = np.where((t < one) & (j < xsize), one - t, ft(0))
        total = total + wt[:, j]
    ws = np.where(total != 0, one / np.where(total != 0, total, one), ft(0)).astype(ft)
    return xmin, xsize, wt * ws[:, None]


def aa_resize(img, win, R, ft=np.float64, mutant=None, swap_rb=False):
    """[R, R, 3] in ft: the window win = (x0, y0, w, h) of the u8 image img [H, W, 3], / 255, resized; taps summed along x then along y."""
    H, W = img.shape[:2]
    x0, y0, w, h = win
    assert 0 <= x0 and 0 <= y0 and w >= 1 and h >= 1 and x0 + w <= W and y0 + h <= H, (win, H, W)
    whole = mutant == "aa_window_reads_image"               # taps clamped to the image: a border tap reads outside the window
    xmin, _, wx = aa_axis(w, R, ft, mutant, *((-x0, W - x0) if whole else (0, w)))
    ymin, _, wy = aa_axis(h, R, ft, mutant, *((-y0, H - y0) if whole else (0, h)))
    v = img.astype(ft) / ft(255)
    if swap_rb:
        v = v[..., ::-1]
    tmp = np.zeros((H, R, 3), ft)
    for j in range(wx.shape[1]):
        tmp = tmp + wx[None, :, j, None] * v[:, np.clip(x0 + xmin + j, 0, W - 1), :]
    acc = np.zeros((R, R, 3), ft)
    for j in range(wy.shape[1]):
        acc = acc + wy[:, j, None, None] * tmp[np.clip(y0 + ymin + j, 0, H - 1)]
    assert acc.dtype == ft
    return acc


def aa_transform_ref(img_u8, R, window=None, swap_rb=False, dtype=torch.float64, mutant=None, stored="f32"):
    """SAM2Transforms.__call__ on one u8 image [H, W, 3] (or its window {x0, y0, w, h}): / 255, antialiased resize to R x R, (x - mean) / std,
    channel-last [R, R, 3] in `dtype`, rounded to the stored type (stored None: as computed)."""
    assert mutant is None or mutant in AA_MUTANTS, mutant
    ft = {torch.float64: np.float64, torch.float32: np.float32}[dtype]
    img = np.asarray(img_u8)
    win = (0, 0, img.shape[1], img.shape[0]) if window is None else tuple(window)
    acc = aa_resize(img, win, R, ft, mutant, swap_rb)
    moved = swap_rb and mutant == "aa_swap_moves_mean_std"  # mean / std follow the source channel
    mean = np.array(MEAN[::-1] if moved else MEAN).astype(ft)
    std = np.array(STD[::-1] if moved else STD).astype(ft)
    y = torch.from_numpy(np.ascontiguousarray((acc - mean) / std))
    return y if stored is None else rT(y, stored)


def aa_interpolate_ref(img_u8, R, window=None, swap_rb=False):
    """The same through torch's own antialiased resize in float64: the cross-check of the statement above."""
    img = torch.from_numpy(np.asarray(img_u8))
    if window is not None:
        x0, y0, w, h = window
        img = img[y0:y0 + h, x0:x0 + w]
    x = img.double().permute(2, 0, 1)[None] / 255
    if swap_rb:
        x = x.flip(1)
    y = F.interpolate(x, size=(R, R), mode="bilinear", antialias=True, align_corners=False)[0].permute(1, 2, 0)
    return (y - torch.tensor(MEAN, dtype=torch.float64)) / torch.tensor(STD, dtype=torch.float64)


# ---- operands and references of a transform row ----------------------------------------------------------------------------------------------------
def _row(rid):
    from op_matrix import RESAMPLE_ROWS
    return next(r for r in RESAMPLE_ROWS if r["id"] == rid)


@functools.lru_cache(maxsize=None)
def tf_images(rid):
    """The row's source images (numpy u8 [H, W, 3]): seeded noise; fill "window": mid-grey noise inside the image's window (its first item) and
    0 / 255 outside it, so that a tap outside the window shows.  Computed once per process, never modified."""
    row = _row(rid)
    g = _gen(rid)
    out = []
    for k, (H, W) in enumerate(row["images"]):
        if row["fill"] == "window":
            img = torch.randint(0, 2, (H, W, 3), generator=g, dtype=torch.uint8) * 255
            _, x0, y0, w, h = next(it for it in row["items"] if it[0] == k)
            x0, y0, w, h = clip_window((x0, y0, w, h), H, W)
            img[y0:y0 + h, x0:x0 + w] = torch.randint(96, 160, (h, w, 3), generator=g, dtype=torch.uint8)
        else:
            img = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8)
        out.append(img.numpy())
    return tuple(out)


def tf_items(row, mutant=None):
    """[(image, clipped window)] of the outputs a launch of the row must produce, in order."""
    items = list(row["items"])
    if mutant == "aa_second_window_table_restarts":         # the second 64-entry table reads the first table's sources again
        from op_matrix import RECT_MAX
        assert len(items) > RECT_MAX, "aa_second_window_table_restarts needs a second table"
        items = [items[b % RECT_MAX] for b in range(len(items))]
    out = []
    for k, x0, y0, w, h in items:
        H, W = row["images"][k]
        out.append((k, clip_window((x0, y0, w, h), H, W, mutant if mutant in CLIP_MUTANTS else None)))
    return out


def _tf_reference(rid, swap, dtype, mutant):
    row = _row(rid)
    imgs = tf_images(rid)
    aam = mutant if mutant in AA_MUTANTS else None
    return torch.stack([aa_transform_ref(imgs[k], row["R"], win, bool(swap), dtype, aam, None) for k, win in tf_items(row, mutant)])


@functools.lru_cache(maxsize=None)
def tf_reference(rid, swap, chain32=False):
    """[items, R, R, 3]: every output of the row, unrounded, in float64 (or the fp32 chain).  Once per process, shared, never modified."""
    return _tf_reference(rid, swap, torch.float32 if chain32 else torch.float64, None)


def tf_mutant(rid, swap, mutant):
    return _tf_reference(rid, swap, torch.float64, mutant)


def tf_runs(row):
    """The forms of a transform row that launch (the others are refused)."""
    return tuple(f for f in row["forms"] if f not in row["refuse"])


# ---- the mask return ---------------------------------------------------------------------------------------------------------------------------------
def bil_explicit(low, H, W, dtype=torch.float64, mutant=None):
    """Bilinear resize [N, h, w] -> [N, H, W], align_corners False, stated per axis: s = max((d + 0.5) in / out - 0.5, 0), i0 = min((int)s, in - 1),
    i1 = min(i0 + 1, in - 1), weight of i1 = s - i0."""
    assert mutant in (None, "bil_align_corners", "bil_no_low_clamp"), mutant
    low = low.to(dtype)

    def axis(n_in, n_out):
        d = torch.arange(n_out, dtype=dtype)
        if mutant == "bil_align_corners":
            s = d * ((n_in - 1) / (n_out - 1) if n_out > 1 else 0.0)
        else:
            s = (d + 0.5) * (torch.tensor(n_in, dtype=dtype) / torch.tensor(n_out, dtype=dtype)) - 0.5
            if mutant != "bil_no_low_clamp":
                s = s.clamp(min=0)
        i0 = s.trunc().long().clamp(max=n_in - 1)           # (int)s of a negative s is 0: the mutant extrapolates below pixel 0
        return i0, (i0 + 1).clamp(max=n_in - 1), s - i0.to(dtype)

    y0, y1, ly = axis(low.shape[1], H)
    x0, x1, lx = axis(low.shape[2], W)
    ly, lx = ly[None, :, None], lx[None, None, :]
    top = (1 - lx) * low[:, y0][:, :, x0] + lx * low[:, y0][:, :, x1]
    bot = (1 - lx) * low[:, y1][:, :, x0] + lx * low[:, y1][:, :, x1]
    return (1 - ly) * top + ly * bot


def mask_ref(low, H, W, dtype=torch.float64, mutant=None):
    return bil_explicit(low, H, W, dtype, mutant) if mutant in ("bil_align_corners", "bil_no_low_clamp") else bilinear_ref(low, H, W, dtype)


def mask_expected(ref, thresh, mutant=None):
    """(u8 mask, extent) of one reference [N, H, W] at a threshold."""
    m, e = mask_and_extent(ref, thresh)
    if mutant == "bil_extent_exclusive_max":                # x1, y1 one past the last pixel
        e = e.clone()
        e[e[:, 2] >= 0, 2:] += 1
    return m, e


@functools.lru_cache(maxsize=None)
def mask_operands(rid):
    """The f32 source planes [N, h, w] of a mask-return row: one blob per plane on a negative background, as helper_ref.operands builds them (two
    planes per seed; kind "edge": rolled so that the blob sits on the borders, where the axis clamps act on the mask), or an empty and a full plane.
    Once per process, never modified."""
    row = _row(rid)
    N, h, w = row["N"], row["h"], row["w"]
    if row.get("kind") == "flat":
        assert N == 2
        return torch.cat((torch.full((1, h, w), -5.0), torch.full((1, h, w), 5.0)))
    parts = [helper_operands(dict(op="bilinear", N=2, h=h, w=w, seed=row["seed"] + 1000 * k), "f32")["low"] for k in range((N + 1) // 2)]
    low = torch.cat(parts)[:N].contiguous()
    if row.get("kind") == "edge":                            # the blob's centre moved to pixel (0, 0): the blob wraps round every border
        for n in range(N):
            low[n] = torch.roll(low[n], (-int(h * (0.35 + 0.3 * (n % 2))), -int(w * (0.6 - 0.25 * (n % 2)))), (0, 1))
    return low


def mask_sizes(row):
    """(H, W) of every plane the row returns (None for a size the entry point must refuse)."""
    if row["op"] == "mask":
        return [(row["H"], row["W"])] * row["N"]
    if row["op"] == "mask_sizes":
        return [s if s[0] > 0 and s[1] > 0 else None for s in row["sizes"]]
    return [clip_plane(rc, row["plane_stride"]) for rc in row["windows"]]


def _mask_planes(rid, dtype, mutant):
    row = _row(rid)
    low = mask_operands(rid)
    bm = mutant if mutant in ("bil_align_corners", "bil_no_low_clamp") else None
    return tuple(None if s is None else mask_ref(low[n:n + 1], s[0], s[1], dtype, bm) for n, s in enumerate(mask_sizes(row)))


@functools.lru_cache(maxsize=None)
def mask_planes(rid, chain32=False):
    """One reference [1, H_n, W_n] per plane of a mask-return row.  Once per process, shared, never modified."""
    return _mask_planes(rid, torch.float32 if chain32 else torch.float64, None)


def mask_planes_mutant(rid, mutant):
    return _mask_planes(rid, torch.float64, mutant)


def extent_planes(row):
    """The u8 planes [N, H, W] of a cvmi_mask_extent row: 255 at the listed (x, y)."""
    m = torch.zeros(len(row["planes"]), row["H"], row["W"], dtype=torch.uint8)
    for n, pts in enumerate(row["planes"]):
        for x, y in pts:
            m[n, y, x] = 255
    return m


# ---- the measurements behind CHAIN32_DEV --------------------------------------------------------------------------------------------------------------
def measure_chain32():
    """{family: largest |chain32 - ref64|} over every row that launches, on the f32 outputs."""
    from op_matrix import RESAMPLE_ROWS
    dev = {"aa_transform": 0.0, "bilinear_edge": 0.0}
    for row in RESAMPLE_ROWS:
        if row["op"] == "transform" and tf_runs(row):
            for swap in row["swaps"]:
                d = float((tf_reference(row["id"], swap, True).double() - tf_reference(row["id"], swap)).abs().max())
                dev["aa_transform"] = max(dev["aa_transform"], d)
        elif row["op"] in ("mask", "mask_sizes", "mask_rects_dev"):
            for a, b in zip(mask_planes(row["id"], True), mask_planes(row["id"])):
                if b is not None:
                    dev["bilinear_edge"] = max(dev["bilinear_edge"], float((a.double() - b).abs().max()))
    return dev


if __name__ == "__main__":
    for fam, d in sorted(measure_chain32().items()):
        print(f"{fam}: largest |chain32 - ref64| {d:.4e}   CHAIN32_DEV {CHAIN32_DEV[fam]:.4e}   ATOL {ATOL[fam]:.4e}")
