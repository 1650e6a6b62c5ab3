"""Automatic mask generation: upstream's `SAM2AutomaticMaskGenerator` at its defaults (one full-image crop, multimask output, no
mask-to-mask pass, no small-region removal) on `SAM2Model`'s encode / decode split.  A regular grid of foreground clicks is decoded in
chunks from ONE embedding (`encode_images`, then `infer_masks(emb, points=...)` per chunk); every candidate plane is scored at the image's
own resolution by cvmi_amg_score -- the two stability counts, the area and the bounding box of the bilinearly resized logits, without the
resized map --, filtered and appended on the device (cvmi_amg_select), de-duplicated by cvmi_yolo_nms on the boxes, and only the survivors
are turned into masks (cvmi_amg_score's mask mode, so `area` and `bbox` describe `segmentation` by construction)."""
import numpy as np
import torch

from . import _lib, amg_utils
from .sam2_infer import SAM2Transforms, Sam2Embeddings

OUTPUT_KEYS = ("segmentation", "area", "bbox", "predicted_iou", "point_coords", "stability_score", "crop_box")
NMS_MAX_DET = 4096                               # cvmi_yolo_nms keeps at most this many boxes per image
POOL_BYTES_IN_FLIGHT = 4 << 30                   # images are processed in sub-batches whose candidate pools stay below this


def build_point_grid(n):
    """upstream's build_point_grid: n x n points in [0, 1]^2 (float64 [n * n, 2] of (x, y), x fastest), offset 1 / (2 n) from the border."""
    offset = 1.0 / (2 * n)
    side = np.linspace(offset, 1.0 - offset, n)
    return np.stack([np.tile(side[None, :], (n, 1)), np.tile(side[:, None], (1, n))], axis=-1).reshape(-1, 2)


class Sam2AutomaticMaskGenerator:
    """`generate(image)` -> list of dicts with upstream's keys, in NMS order (predicted IoU descending):
      segmentation  u8 {0, 255} [H, W] on the device (`.bool()` is upstream's array),   area  its pixel count,
      bbox  [x0, y0, x1 - x0, y1 - y0] of the inclusive extent (upstream's box_xyxy_to_xywh of batched_mask_to_box, quirk included),
      predicted_iou,  stability_score = #(v > t + offset) / #(v > t - offset) in f32,  point_coords [[x, y]] = the grid point in original
      pixels,  crop_box [0, 0, W, H].
    A candidate is kept iff predicted_iou > pred_iou_thresh and stability_score >= stability_score_thresh; greedy box NMS (IoU >
    box_nms_thresh suppresses, ties to the lower candidate index, boxes taken as the floats of the inclusive corners) removes duplicates.
    Scoring runs on the decoder's low-res logits resized bilinearly to (H, W) -- upstream's predictor with return_logits=True; the refinement
    head is not run.

    max_candidates (default min(3 * points, 4096)): slots of the per-image pool that holds the kept candidates' low-res planes until NMS has
    run -- (R / 4)^2 * 4 bytes each, 256 KB at R = 1024, so at most 1 GB per image in flight; images are processed in sub-batches that keep
    the pools below 4 GB.  More kept candidates than slots raise RuntimeError (nothing is dropped silently); NMS returns at most 4096 masks.

    The host waits once per sub-batch of `generate_batch` for what this class launches: after the last chunk and the NMS are enqueued, to
    read the kept counts and the records.  (`infer_masks` itself synchronises its stream at the end of every call, as for every caller; no
    value travels through the host between the chunks.)

    Two of upstream's constructor options are PER-CALL arguments of `generate` / `generate_batch` here, so that one generator and one plan
    serve a different output form per request (the constructor still refuses them, with `crop_n_layers`, `use_m2m` and a non-default
    `output_mode`):
      min_mask_region_area > 0   upstream's postprocess_small_regions after the first NMS (amg_utils.py: holes below the area filled, then
                                 islands below it removed, on the GPU; every box recomputed; a second box NMS with box_nms_thresh in which an
                                 unchanged mask outranks a changed one).  The list comes back in that NMS's order -- unchanged masks first, each
                                 group by predicted IoU -- and `segmentation`, `area`, `bbox` describe the final plane.
      output_mode                "binary_mask" (default), or "uncompressed_rle": `segmentation` = {"size": [H, W], "counts": [...]} (column-major
                                 runs starting with a run of zeros; amg_utils.rle_to_mask decodes), `area` = amg_utils.area_from_rle of it.  The
                                 H x W planes are then built and encoded in chunks of at most amg_utils.MASK_CHUNK_BYTES and never all held.
                                 "coco_rle" raises NotImplementedError: its string form is pycocotools', which is not available to check against.
    With both at their defaults the path is the one above: no extra launch, no extra wait.  Otherwise everything either option needs is
    enqueued for all images of the sub-batch -- the planes, cvmi_mask_remove_small, the second cvmi_yolo_nms, cvmi_mask_rle with a capacity
    guess -- and the host waits ONCE more per sub-batch, for the second NMS's keep lists and the planes' info (min_mask_region_area) and
    the RLE offsets and counts (uncompressed_rle) together: one added wait whichever options are set.  A chunk of planes with more than
    amg_utils.RLE_RUNS_PER_COLUMN runs per column on average is encoded a second time with the exact capacity, with a wait of its own."""

    def __init__(self, model, points_per_side=32, points_per_batch=64, pred_iou_thresh=0.8, stability_score_thresh=0.95,
                 stability_score_offset=1.0, mask_threshold=0.0, box_nms_thresh=0.7, point_grids=None, multimask_output=True, max_candidates=None,
                 output_mode="binary_mask", crop_n_layers=0, min_mask_region_area=0, use_m2m=False):
        if crop_n_layers > 0:
            raise NotImplementedError("crop_n_layers > 0: only the single full-image crop is built")
        if min_mask_region_area > 0:
            raise NotImplementedError("min_mask_region_area > 0 is a per-call argument here: generate(image, min_mask_region_area=...) / "
                                      "generate_batch(..., min_mask_region_area=...), or amg_utils.postprocess_small_regions on a returned list")
        if use_m2m:
            raise NotImplementedError("use_m2m=True: the mask-to-mask refinement pass is not built")
        if output_mode != "binary_mask":
            raise NotImplementedError(f"output_mode={output_mode!r} is a per-call argument here: generate(image, output_mode='uncompressed_rle') / "
                                      "generate_batch(..., output_mode=...), or amg_utils.mask_to_rle on returned planes ('coco_rle' is not built)")
        if (points_per_side is None) == (point_grids is None):
            raise ValueError("exactly one of points_per_side and point_grids must be given")
        if point_grids is not None:
            if len(point_grids) != 1:
                raise ValueError("point_grids: one grid (crop_n_layers = 0)")
            grid = np.asarray(point_grids[0], dtype=np.float64)
            if grid.ndim != 2 or grid.shape[1] != 2 or grid.shape[0] == 0:
                raise ValueError("point_grids[0] must be [n, 2] points in [0, 1]^2")
        else:
            if int(points_per_side) <= 0:
                raise ValueError("points_per_side must be positive")
            grid = build_point_grid(int(points_per_side))
        if int(points_per_batch) <= 0:
            raise ValueError("points_per_batch must be positive")
        if not pred_iou_thresh >= 0:
            raise ValueError("pred_iou_thresh must be >= 0 (cvmi_yolo_nms sorts non-negative scores)")
        self.model, self.grid = model, grid
        self.points_per_batch = int(points_per_batch)
        self.pred_iou_thresh, self.stability_score_thresh = float(pred_iou_thresh), float(stability_score_thresh)
        self.stability_score_offset, self.mask_threshold, self.box_nms_thresh = float(stability_score_offset), float(mask_threshold), float(box_nms_thresh)
        self.multimask_output = bool(multimask_output)
        self.ncand = 3 if self.multimask_output else 1
        self.cap = int(max_candidates) if max_candidates is not None else min(self.ncand * len(grid), 4096)
        if self.cap <= 0:
            raise ValueError("max_candidates must be positive")
        self.transforms = SAM2Transforms(model.image_size, self.mask_threshold)
        # the three levels, in double, rounded once to f32 (by the C ABI's float arguments)
        self.levels = (self.mask_threshold - self.stability_score_offset, self.mask_threshold, self.mask_threshold + self.stability_score_offset)
        # what the decoder sees: norm * R in f32
        self.points_in = torch.from_numpy(grid.astype(np.float32)) * float(model.image_size)

    # -- public surface
    def generate(self, image, min_mask_region_area=0, output_mode="binary_mask"):
        """image: RGB u8 [H, W, 3] (array or PIL) -> list of dicts.  min_mask_region_area, output_mode: see the class."""
        img = self.transforms._check_u8(image)
        return self.generate_batch([img], min_mask_region_area=min_mask_region_area, output_mode=output_mode)[0]

    def generate_batch(self, images, orig_hw=None, min_mask_region_area=0, output_mode="binary_mask"):
        """images: a list of RGB u8 [H, W, 3] images (orig_hw then defaults to their sizes), a [B, 3, R, R] tensor as `infer_masks` takes it, or
        the `Sam2Embeddings` `encode_images` made of one; orig_hw = [(H, W)] per image.  -> one list of dicts per image."""
        model = self.model
        if output_mode == "coco_rle":
            raise NotImplementedError("output_mode='coco_rle': the compressed string form is pycocotools', which is not available to check an "
                                      "encoder against; 'uncompressed_rle' carries the same runs")
        if output_mode not in ("binary_mask", "uncompressed_rle"):
            raise ValueError(f"output_mode must be 'binary_mask' or 'uncompressed_rle', not {output_mode!r}")
        min_area = int(min_mask_region_area)
        if min_area < 0:
            raise ValueError("min_mask_region_area must be >= 0")
        if isinstance(images, (list, tuple)):
            imgs = [self.transforms._check_u8(im) for im in images]
            if orig_hw is None:
                orig_hw = [im.shape[:2] for im in imgs]
            images = self.transforms.forward_batch(imgs) if imgs else None
        if orig_hw is None:
            raise ValueError("orig_hw = [(H, W)] per image is required with a tensor or embeddings")
        B = len(images) if isinstance(images, Sam2Embeddings) else (0 if images is None else int(images.shape[0]))
        sizes = [(int(s[0]), int(s[1])) for s in orig_hw]
        if len(sizes) != B:
            raise ValueError(f"orig_hw names {len(sizes)} sizes for {B} images")
        if any(H <= 0 or W <= 0 for H, W in sizes):
            raise ValueError("orig_hw: sizes must be positive")
        if B == 0:
            return []
        f0 = model.image_size // 4
        step = max(1, POOL_BYTES_IN_FLIGHT // (self.cap * f0 * f0 * 4))
        out = []
        for a in range(0, B, step):
            src = images[a:a + step]
            emb = src if isinstance(src, Sam2Embeddings) else model.encode_images(src)
            out += self._generate(emb, sizes[a:a + step], min_area, output_mode)
        return out

    # -- one sub-batch
    def _candidates(self, emb, sizes):
        """Enqueue every chunk of the grid for the images of `emb`: decode, score, filter + append.  -> the per-image device state
        (counter i32 [B, 2], records i32 [B, cap, 10], pool f32 [B, cap, R/4, R/4], block f32 [B, 5, cap]); nothing is read back."""
        lib, model = _lib.load(), self.model
        B, cap, C, Pb = len(emb), self.cap, self.ncand, self.points_per_batch
        f0 = model.image_size // 4
        lo, mid, hi = self.levels
        dev = emb.device
        sp = torch.cuda.current_stream().cuda_stream
        counter = torch.zeros(B, 2, dtype=torch.int32, device=dev)
        records = torch.zeros(B, cap, len(_lib.AMG_RECORD), dtype=torch.int32, device=dev)
        pool = torch.empty(B, cap, f0, f0, dtype=torch.float32, device=dev)
        block = torch.zeros(B, 5, cap, dtype=torch.float32, device=dev)
        block[:, 4].fill_(float("-inf"))                                         # unused columns never pass the NMS's conf_thres
        stats = torch.empty(B, Pb * C, 8, dtype=torch.int32, device=dev)
        labels = torch.ones(B, Pb, 1, dtype=torch.int32)
        for base in range(0, len(self.grid), Pb):
            pts = self.points_in[base:base + Pb]
            n_valid = pts.shape[0]
            if n_valid < Pb:                                                     # a short last chunk: the last point repeated, never selected
                pts = torch.cat([pts, pts[-1:].expand(Pb - n_valid, 2)])
            _, low, iou = model.infer_masks(emb, points=pts.view(1, Pb, 1, 2).expand(B, Pb, 1, 2), point_labels=labels,
                                            multimask_output=self.multimask_output, return_high_res=False)
            low, iou = low.view(B, Pb * C, f0, f0), iou.view(B, Pb * C)
            for b, (H, W) in enumerate(sizes):
                _lib.check(lib.cvmi_amg_score(low[b].data_ptr(), Pb * C, f0, f0, H, W, lo, mid, hi, stats[b].data_ptr(), None, sp), "amg_score")
                _lib.check(lib.cvmi_amg_select(stats[b].data_ptr(), iou[b].data_ptr(), low[b].data_ptr(), Pb * C, n_valid * C, C, base,
                                               self.pred_iou_thresh, self.stability_score_thresh, f0 * f0, cap, counter[b].data_ptr(),
                                               records[b].data_ptr(), pool[b].data_ptr(), block[b].data_ptr(), sp), "amg_select")
        return dict(counter=counter, records=records, pool=pool, block=block)

    def _generate(self, emb, sizes, min_area=0, output_mode="binary_mask"):
        """Candidates, NMS, the single host wait, then the survivors' masks."""
        lib, model = _lib.load(), self.model
        B, cap, f0 = len(emb), self.cap, model.image_size // 4
        lo, mid, hi = self.levels
        dev = emb.device
        with torch.cuda.device(dev):
            sp = torch.cuda.current_stream().cuda_stream
            st = self._candidates(emb, sizes)
            counter, records, pool, block = st["counter"], st["records"], st["pool"], st["block"]
            max_det = min(cap, NMS_MAX_DET)
            ws = torch.empty(int(lib.cvmi_yolo_nms_workspace(B, cap)), dtype=torch.uint8, device=dev)
            det = torch.empty(B, max_det, 6, dtype=torch.float32, device=dev)
            keep_idx = torch.empty(B, max_det, dtype=torch.int32, device=dev)
            keep_n = torch.empty(B, dtype=torch.int32, device=dev)
            _lib.check(lib.cvmi_yolo_nms(block.data_ptr(), B, 1, cap, self.pred_iou_thresh, self.box_nms_thresh, max_det, 0.0, det.data_ptr(),
                                         keep_idx.data_ptr(), keep_n.data_ptr(), ws.data_ptr(), sp), "yolo_nms")
            # the one wait: counts, kept indices and records in pinned buffers, one synchronise
            host = [torch.empty(t.shape, dtype=t.dtype, pin_memory=True) for t in (counter, keep_n, keep_idx, records)]
            for h, t in zip(host, (counter, keep_n, keep_idx, records)):
                h.copy_(t, non_blocking=True)
            torch.cuda.current_stream().synchronize()
            counts, kept_n, kept_idx, recs = (h.numpy() for h in host)
            recs = recs.view(_lib.AMG_RECORD).reshape(B, cap)
            if int(counts[:, 0].max()) > cap:
                raise RuntimeError(f"{int(counts[:, 0].max())} candidates passed the filters but max_candidates = {cap}: raise max_candidates "
                                   "(or the thresholds)")
            if min_area > 0 or output_mode != "binary_mask":
                return self._finish_with_options(sizes, pool, keep_idx, kept_n, kept_idx, recs, min_area, output_mode)
            out = []
            for b, (H, W) in enumerate(sizes):
                K = int(kept_n[b])
                if K == 0:
                    out.append([])
                    continue
                planes = pool[b].index_select(0, keep_idx[b, :K].long())
                masks = torch.empty(K, H, W, dtype=torch.uint8, device=dev)
                fstats = torch.empty(K, 8, dtype=torch.int32, device=dev)                  # equal to the records' by construction; not read back
                _lib.check(lib.cvmi_amg_score(planes.data_ptr(), K, f0, f0, H, W, lo, mid, hi, fstats.data_ptr(), masks.data_ptr(), sp), "amg_score")
                dicts = []
                for k in range(K):
                    r = recs[b, int(kept_idx[b, k])]
                    x0, y0, x1, y1 = int(r["x0"]), int(r["y0"]), int(r["x1"]), int(r["y1"])
                    gx, gy = self.grid[int(r["point"])]
                    dicts.append({"segmentation": masks[k], "area": int(r["area"]), "bbox": [x0, y0, x1 - x0, y1 - y0],
                                  "predicted_iou": float(r["score"]), "point_coords": [[float(gx * W), float(gy * H)]],
                                  "stability_score": float(r["stability"]), "crop_box": [0, 0, W, H]})
                out.append(dicts)
            return out

    # -- the per-call options
    def _masks(self, low_planes, H, W):
        """u8 [K, H, W] planes of the kept candidates' low-res planes (cvmi_amg_score's mask mode), enqueued."""
        lib, f0 = _lib.load(), self.model.image_size // 4
        lo, mid, hi = self.levels
        K = int(low_planes.shape[0])
        masks = torch.empty(K, H, W, dtype=torch.uint8, device=low_planes.device)
        fstats = torch.empty(K, 8, dtype=torch.int32, device=low_planes.device)
        _lib.check(lib.cvmi_amg_score(low_planes.data_ptr(), K, f0, f0, H, W, lo, mid, hi, fstats.data_ptr(), masks.data_ptr(),
                                      torch.cuda.current_stream().cuda_stream), "amg_score")
        return masks

    def _finish_with_options(self, sizes, pool, keep_idx, kept_n, kept_idx, recs, min_area, output_mode):
        """After the first NMS's wait: per image the survivors' planes (all of them, or chunk by chunk in the RLE mode), small-region removal,
        the second NMS and the encoding are enqueued; ONE wait for the whole sub-batch; then the dicts."""
        rle = output_mode == "uncompressed_rle"
        work = []
        for b, (H, W) in enumerate(sizes):
            K = int(kept_n[b])
            if K == 0:
                work.append(None)
                continue
            low = pool[b].index_select(0, keep_idx[b, :K].long())
            step = max(1, amg_utils.MASK_CHUNK_BYTES // (H * W)) if rle else K
            masks, infos, pending = None, [], []
            for a in range(0, K, step):
                def build(a=a, H=H, W=W, low=low, step=step):
                    m = self._masks(low[a:a + step], H, W)
                    return m, (amg_utils.remove_small_enqueue(m, min_area, amg_utils.PHASES["both"]) if min_area > 0 else None)
                masks, info = build()
                infos.append(info)
                if rle:
                    pending.append(amg_utils.PendingRle(masks, rebuild=lambda build=build: build()[0]))
                    masks = None                                                 # the chunk's planes are free again once the stream has passed them
            nms = amg_utils.SecondNms(torch.cat(infos), self.box_nms_thresh) if min_area > 0 else None
            work.append((K, masks, pending, nms))
        torch.cuda.current_stream().synchronize()
        out = []
        for b, (H, W) in enumerate(sizes):
            if work[b] is None:
                out.append([])
                continue
            K, masks, pending, nms = work[b]
            order, info = nms.finish() if nms is not None else (range(K), None)
            segs = [r for p in pending for r in p.finish()] if rle else masks
            dicts = []
            for k in order:
                r = recs[b, int(kept_idx[b, k])]
                x0, y0, x1, y1 = int(r["x0"]), int(r["y0"]), int(r["x1"]), int(r["y1"])
                gx, gy = self.grid[int(r["point"])]
                d = {"segmentation": segs[k], "area": int(r["area"]), "bbox": [x0, y0, x1 - x0, y1 - y0],
                     "predicted_iou": float(r["score"]), "point_coords": [[float(gx * W), float(gy * H)]],
                     "stability_score": float(r["stability"]), "crop_box": [0, 0, W, H]}
                dicts.append(amg_utils.survivor(d, segs[k], info[k]) if info is not None else d)
            out.append(dicts)
        return out
