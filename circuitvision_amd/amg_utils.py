"""The mask utilities of upstream's `sam2/utils/amg.py` on device tensors: uncompressed RLE (csrc/mask_rle.hip, cvmi_mask_rle), small-region
removal (csrc/mask_cc.hip, cvmi_mask_remove_small) and `postprocess_small_regions` on both plus a second box NMS (cvmi_yolo_nms).  Names and
meanings are upstream's; where upstream loops over masks, these take a stack [K, H, W] of u8 planes (foreground = a non-zero byte).  The crop
geometry of the generator's crop layers is here too, on the host: `build_point_grid`, `build_all_layer_point_grids`, `generate_crop_boxes`.

An RLE is `{"size": [H, W], "counts": [int, ...]}`: the plane read in column-major order (y fastest), runs alternating and starting with a
run of zeros (0 when pixel (0, 0) is set), a run going on across a column end, the runs summing to H * W.

`changed` is true where a pixel of the plane was filled or removed.  (Upstream's flag is "a small region was found", which differs in one
case: a plane whose only foreground component is small keeps it -- no pixel changes -- and upstream still reports a change.)"""
import numpy as np
import torch

from . import _lib

REMOVE_SMALL_WORKSPACE_BYTES = 1 << 30           # cvmi_mask_remove_small runs on chunks of planes whose two ints per pixel stay below this (128 planes at 1024 x 1024)
MASK_CHUNK_BYTES = 1 << 30                       # u8 planes a caller that encodes in chunks holds at a time (amg.py's RLE mode)
RLE_RUNS_PER_COLUMN = 4                          # the capacity guess of mask_to_rle: K * (4 W + 2) runs; a stack with more is encoded twice
NMS_MAX_DET, NMS_MAX_A = 4096, 65536             # cvmi_yolo_nms keeps at most this many boxes, of at most this many
PHASES = {"holes": 1, "islands": 2, "both": 3}
INFO = ("changed", "area", "x0", "y0", "x1", "y1", "filled", "removed")


# ---- crop geometry (host) -------------------------------------------------------------------------------------------------------------------------
def build_point_grid(n):
    """upstream's build_point_grid: n x n points in [0, 1]^2 (float64 [n * n, 2] of (x, y), x fastest), offset 1 / (2 n) from the border."""
    offset = 1.0 / (2 * n)
    side = np.linspace(offset, 1.0 - offset, n)
    return np.stack([np.tile(side[None, :], (n, 1)), np.tile(side[:, None], (1, n))], axis=-1).reshape(-1, 2)


def build_all_layer_point_grids(n_per_side, n_layers, scale_per_layer):
    """upstream's build_all_layer_point_grids: the grid of layer i has int(n_per_side / scale_per_layer ** i) points per side, i = 0 .. n_layers.
    A layer left without a point raises ValueError (upstream would divide by zero)."""
    grids = []
    for i in range(int(n_layers) + 1):
        n = int(n_per_side / (scale_per_layer ** i))
        if n <= 0:
            raise ValueError(f"crop layer {i}: int({n_per_side} / {scale_per_layer} ** {i}) = {n} points per side")
        grids.append(build_point_grid(n))
    return grids


def generate_crop_boxes(im_size, n_layers, overlap_ratio):
    """upstream's generate_crop_boxes: im_size = (H, W) -> (boxes [[x0, y0, x1, y1]] with exclusive ends, layer_idxs).  Box 0 is the image,
    layer 0; layer i + 1 has (2 ** (i + 1)) ** 2 overlapping crops, x outer and y inner."""
    import itertools
    import math
    H, W = int(im_size[0]), int(im_size[1])
    boxes, layer_idxs = [[0, 0, W, H]], [0]
    for i in range(int(n_layers)):
        n = 2 ** (i + 1)
        overlap = int(overlap_ratio * min(H, W) * (2 / n))
        crop_w, crop_h = (int(math.ceil((overlap * (n - 1) + length) / n)) for length in (W, H))
        x0s = [int((crop_w - overlap) * k) for k in range(n)]
        y0s = [int((crop_h - overlap) * k) for k in range(n)]
        for x0, y0 in itertools.product(x0s, y0s):
            boxes.append([x0, y0, min(x0 + crop_w, W), min(y0 + crop_h, H)])
            layer_idxs.append(i + 1)
    return boxes, layer_idxs


def _planes(masks):
    if not (isinstance(masks, torch.Tensor) and masks.is_cuda and masks.dtype == torch.uint8 and masks.dim() == 3 and masks.is_contiguous()):
        raise ValueError("masks must be a contiguous u8 [K, H, W] tensor on the device")
    K, H, W = (int(v) for v in masks.shape)
    if K and (H <= 0 or W <= 0):
        raise ValueError("masks: H and W must be positive")
    return K, H, W


def _pinned(t):
    """An asynchronous copy of a device tensor to pinned memory: valid after the stream is synchronised."""
    h = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
    h.copy_(t, non_blocking=True)
    return h


# ---- RLE ------------------------------------------------------------------------------------------------------------------------------------------
class PendingRle:
    """cvmi_mask_rle enqueued on the current stream with a capacity guess, offsets and counts on their way to pinned memory; `finish()`,
    after the stream has been synchronised, returns the list of RLE dicts -- after ONE repeat with the exact capacity (and a wait of its own)
    where the guess was too small.  rebuild: a callable that returns the planes again for that repeat, so that they need not be held."""

    def __init__(self, masks, rebuild=None):
        self.K, self.H, self.W = _planes(masks)
        self.masks, self.rebuild = (None, rebuild) if rebuild is not None else (masks, None)
        self.cap = min(self.K * (RLE_RUNS_PER_COLUMN * self.W + 2), self.K * (self.H * self.W + 1))
        self.host = self._launch(masks, self.cap) if self.K else None

    def _launch(self, masks, cap):
        lib, K, H, W = _lib.load(), self.K, self.H, self.W
        nbytes = int(lib.cvmi_mask_rle_workspace(K, H, W))
        if nbytes == 0:
            raise ValueError(f"mask_to_rle: {K} planes of {H} x {W}: K * H * W + K must be below 2^31")
        with torch.cuda.device(masks.device):
            ws = torch.empty(nbytes, dtype=torch.uint8, device=masks.device)
            offsets = torch.empty(K + 1, dtype=torch.int32, device=masks.device)
            counts = torch.empty(cap, dtype=torch.int32, device=masks.device)
            _lib.check(lib.cvmi_mask_rle(masks.data_ptr(), K, H, W, cap, offsets.data_ptr(), counts.data_ptr(), ws.data_ptr(), nbytes,
                                         torch.cuda.current_stream().cuda_stream), "mask_rle")
            return _pinned(offsets), _pinned(counts)

    def finish(self):
        if not self.K:
            return []
        offsets, counts = (h.numpy() for h in self.host)
        total = int(offsets[-1])
        if total > self.cap:                                                     # the one repeat: the total is known now
            masks = self.masks if self.masks is not None else self.rebuild()
            host = self._launch(masks, total)
            torch.cuda.current_stream(masks.device).synchronize()
            offsets, counts = (h.numpy() for h in host)
            assert int(offsets[-1]) == total
        self.masks = self.rebuild = self.host = None
        return [{"size": [self.H, self.W], "counts": counts[offsets[k]:offsets[k + 1]].tolist()} for k in range(self.K)]


def mask_to_rle(masks):
    """upstream's mask_to_rle_pytorch: u8 [K, H, W] on the device -> a list of K RLE dicts.  One cvmi_mask_rle call with a capacity guess and at most
    one repeat; only `offsets` and `counts` cross to the host."""
    pending = PendingRle(masks)
    if pending.K:
        torch.cuda.current_stream(masks.device).synchronize()
    return pending.finish()


def rle_to_mask(rle):
    """upstream's rle_to_mask: -> bool [H, W] numpy array on the host."""
    H, W = (int(v) for v in rle["size"])
    counts = np.asarray(rle["counts"], dtype=np.int64)
    if counts.size == 0 or (counts < 0).any() or int(counts.sum()) != H * W:
        raise ValueError("rle: the counts must be non-negative and sum to H * W")
    flat = np.repeat(np.arange(counts.size) % 2 == 1, counts)
    return np.ascontiguousarray(flat.reshape(W, H).T)


def area_from_rle(rle):
    """upstream's area_from_rle: the sum of the runs of ones."""
    return int(sum(rle["counts"][1::2]))


# ---- small regions --------------------------------------------------------------------------------------------------------------------------------
def remove_small_enqueue(masks, area_thresh, phases):
    """cvmi_mask_remove_small in place on u8 [K, H, W], in chunks of planes that keep the workspace below REMOVE_SMALL_WORKSPACE_BYTES, on the
    current stream.  -> info i32 [K, 8] on the device (INFO names the columns); nothing is read back."""
    K, H, W = _planes(masks)
    area_thresh, phases = int(area_thresh), int(phases)
    if area_thresh <= 0 or phases not in (1, 2, 3):
        raise ValueError("remove_small_regions: area_thresh must be positive and phases one of 1, 2, 3")
    info = torch.empty(K, len(INFO), dtype=torch.int32, device=masks.device)
    if K == 0:
        return info
    lib = _lib.load()
    step = min(K, max(1, REMOVE_SMALL_WORKSPACE_BYTES // (8 * H * W)))
    nbytes = int(lib.cvmi_mask_remove_small_workspace(step, H, W))
    if nbytes == 0:
        raise ValueError(f"remove_small_regions: {step} planes of {H} x {W}: a chunk must hold fewer than 2^31 pixels")
    with torch.cuda.device(masks.device):
        ws = torch.empty(nbytes, dtype=torch.uint8, device=masks.device)
        sp = torch.cuda.current_stream().cuda_stream
        for a in range(0, K, step):
            _lib.check(lib.cvmi_mask_remove_small(masks[a].data_ptr(), min(step, K - a), H, W, area_thresh, phases, info[a].data_ptr(), ws.data_ptr(), sp),
                       "mask_remove_small")
    return info


def remove_small_regions(masks, area_thresh, mode):
    """upstream's remove_small_regions on a stack, IN PLACE: mode "holes" fills the background components below area_thresh, "islands" removes the
    foreground components below it (the largest stays where every one is small), "both" does the first and then the second on its result.
    -> (masks, changed bool [K] on the device)."""
    if mode not in PHASES:
        raise ValueError(f"mode must be one of {sorted(PHASES)}, not {mode!r}")
    info = remove_small_enqueue(masks, area_thresh, PHASES[mode])
    return masks, info[:, 0] != 0


class SecondNms:
    """The box NMS of postprocess_small_regions, enqueued: boxes = the final planes' extents (info), score 2 for an unchanged plane and 1 for a
    changed one (cvmi_yolo_nms sorts by score, ties to the lower index, so the survivors come unchanged first, each group in its previous
    order).  `finish()`, after the stream has been synchronised -> (kept indices in NMS order, info as an i64 numpy array [K, 8])."""

    def __init__(self, info, nms_thresh):
        lib, K, dev = _lib.load(), int(info.shape[0]), info.device
        if not 0 < K <= NMS_MAX_A:
            raise ValueError(f"postprocess_small_regions: {K} masks; the NMS takes 1 .. {NMS_MAX_A}")
        with torch.cuda.device(dev):
            f = info.to(torch.float32)
            block = torch.stack([(f[:, 2] + f[:, 4]) * 0.5, (f[:, 3] + f[:, 5]) * 0.5, f[:, 4] - f[:, 2], f[:, 5] - f[:, 3], 2.0 - f[:, 0]]).contiguous()
            max_det = min(K, NMS_MAX_DET)
            ws = torch.empty(int(lib.cvmi_yolo_nms_workspace(1, K)), dtype=torch.uint8, device=dev)
            det = torch.empty(max_det, 6, dtype=torch.float32, device=dev)
            keep_idx = torch.empty(max_det, dtype=torch.int32, device=dev)
            keep_n = torch.empty(1, dtype=torch.int32, device=dev)
            _lib.check(lib.cvmi_yolo_nms(block.data_ptr(), 1, 1, K, 0.0, float(nms_thresh), max_det, 0.0, det.data_ptr(), keep_idx.data_ptr(),
                                         keep_n.data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream), "yolo_nms")
            self.host = _pinned(keep_n), _pinned(keep_idx), _pinned(info)

    def finish(self):
        keep_n, keep_idx, info = (h.numpy() for h in self.host)
        return keep_idx[:int(keep_n[0])].tolist(), info.astype(np.int64)


def postprocess_small_regions(dicts, min_area, nms_thresh, output_mode="binary_mask"):
    """upstream's SAM2AutomaticMaskGenerator.postprocess_small_regions on a list as `generate()` returns it (`segmentation` = u8 [H, W] planes on
    the device, all of one size): both phases on copies of the stacked planes, every box recomputed, a second box NMS in which an unchanged
    mask outranks a changed one.  -> the survivors in that NMS order (unchanged first, each group in its previous order) as new dicts:
    `segmentation`, `area` and `bbox` of the final plane; predicted_iou, stability_score, point_coords and crop_box as they were, as upstream
    leaves them.  The input is not modified.  One host wait (the keep list and the planes' info), one more in the RLE mode."""
    if output_mode not in ("binary_mask", "uncompressed_rle"):
        raise ValueError(f"output_mode must be 'binary_mask' or 'uncompressed_rle', not {output_mode!r}")
    dicts = list(dicts)
    if not dicts:
        return []
    masks = torch.stack([d["segmentation"] for d in dicts]).contiguous()
    info = remove_small_enqueue(masks, min_area, PHASES["both"])
    nms = SecondNms(info, nms_thresh)
    torch.cuda.current_stream(masks.device).synchronize()
    keep, info = nms.finish()
    segs = [masks[i] for i in keep]
    if output_mode == "uncompressed_rle" and keep:
        segs = mask_to_rle(masks.index_select(0, torch.as_tensor(keep, dtype=torch.long, device=masks.device)))
    return [survivor(dicts[i], seg, info[i]) for i, seg in zip(keep, segs)]


def survivor(d, segmentation, info_row):
    """The output dict of a mask after small-region removal: its own keys, with segmentation, area and bbox of the final plane."""
    _, area, x0, y0, x1, y1 = (int(v) for v in info_row[:6])
    out = dict(d)
    out.update(segmentation=segmentation, area=area, bbox=[x0, y0, x1 - x0, y1 - y0])
    return out
