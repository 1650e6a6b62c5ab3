"""Automatic mask generation: upstream's `SAM2AutomaticMaskGenerator` at its defaults (one full-image crop, multimask output, no
mask-to-mask pass, no small-region removal) on `SAM2Model`'s encode / decode split.  A regular grid of foreground clicks is decoded in
chunks from ONE embedding (`encode_images`, then `infer_masks(emb, points=...)` per chunk); every candidate plane is scored at the image's
own resolution by cvmi_amg_score -- the two stability counts, the area and the bounding box of the bilinearly resized logits, without the
resized map --, filtered and appended on the device (cvmi_amg_select), de-duplicated by cvmi_yolo_nms on the boxes, and only the survivors
are turned into masks (cvmi_amg_score's mask mode, so `area` and `bbox` describe `segmentation` by construction).

With `crop_n_layers > 0` (a per-call argument) the grid runs again on overlapping crops of the image (amg_utils.generate_crop_boxes): the
crops are source rectangles of ONE uploaded image (cvmi_sam2_transform_srcs), encoded as a batch; the append drops the candidates a crop
border cuts (cvmi_amg_select_crop); a second cvmi_yolo_nms across the crops prefers the smaller crop; and the survivors' masks are written
into a window of a full-image plane (cvmi_amg_score_window).

With `use_m2m=True` (a per-call argument) every chunk's candidates are refined by upstream's mask-to-mask pass before they are scored:
`infer_masks(m2m=True)` replays a second, single-mask decode plan behind the first, fed on the device by cvmi_m2m_fanout."""
import numpy as np
import torch

from . import _lib, amg_utils
from .amg_utils import build_point_grid  # noqa: F401  (upstream's name, kept importable from here)
from .sam2_infer import F32, SAM2Transforms, Sam2Embeddings

OUTPUT_KEYS = ("segmentation", "area", "bbox", "predicted_iou", "point_coords", "stability_score", "crop_box")
NMS_MAX_DET = 4096                               # cvmi_yolo_nms keeps at most this many boxes per image
POOL_BYTES_IN_FLIGHT = 4 << 30                   # images (or crops) are processed in sub-batches whose candidate pools stay below this
M2M_PAIRS_IN_FLIGHT = 1024                       # use_m2m: pairs of a chunk's second decode plan (ncand * points_per_batch per image decoded together)
CROP_EDGE_TOL = 20                               # upstream's is_box_near_crop_edge atol, in pixels


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
    serve a different output form per request (the constructor still refuses them, with `crop_n_layers`, `use_m2m` -- per-call arguments too,
    below -- and a non-default `output_mode`):
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
    amg_utils.RLE_RUNS_PER_COLUMN runs per column on average is encoded a second time with the exact capacity, with a wait of its own.

    The crop options are per-call arguments too (the constructor refuses `crop_n_layers > 0`; the layer grids come from `points_per_side`, so a
    generator built from explicit `point_grids` raises ValueError for them):
      crop_n_layers > 0          upstream's crop layers: layer i has (2 ** i) ** 2 overlapping crops (amg_utils.generate_crop_boxes with
                                 crop_overlap_ratio), each with the grid of int(points_per_side / crop_n_points_downscale_factor ** i) points
                                 per side.  The input must be a list of u8 images (the crops need the pixels); each image is processed on its own:
                                 uploaded once, its crops encoded and decoded in sub-batches that keep the pools below 4 GB, the crops of a
                                 sub-batch that share a layer decoded together.  Per crop the pipeline is the one above, in the crop's
                                 coordinates, plus upstream's border filter: a candidate whose box has a side within 20 pixels of a crop
                                 side that is not within 20 pixels of the image's side is dropped before the per-crop NMS.
      crop_nms_thresh            the box NMS across the crops, on the per-crop survivors in (crop order, per-crop NMS order) with score
                                 1 / (crop area) in f32: a mask of a smaller crop outranks one of a larger crop, and -- this project's rule, the
                                 kernel's -- equal scores go to the lower index, i.e. the earlier crop and within it the per-crop NMS order.  The
                                 list comes back in that NMS's order.  A single crop box has no such NMS, as upstream.  More than 4096 per-crop
                                 survivors in total raise RuntimeError.
    `segmentation`, `area`, `bbox` and `point_coords` are in the ORIGINAL image's coordinates (point_coords = [[gx * cw + cx0, gy * ch + cy0]]
    for the crop [cx0, cy0, cw, ch], which is `crop_box`).  Both options above compose with crops; the second NMS of min_mask_region_area then
    uses max(box_nms_thresh, crop_nms_thresh), upstream's rule.  The host waits, per image: once per sub-batch of crops (as above), once after
    the cross-crop NMS for its keep list, and the options' one extra wait.  With crop_n_layers == 0 nothing of this runs.

    The mask-to-mask pass is a per-call argument as well (the constructor refuses `use_m2m=True` and points here):
      use_m2m=True               upstream's refine_with_m2m: every candidate of a chunk -- before anything is filtered -- goes back to the decoder
                                 as its own mask prompt (its logits clamped to [-32, 32], beside the grid point it came from) in ONE single-mask
                                 pass, inside the chunk's `infer_masks(m2m=True)` call: no extra host wait, no extra upload.  The refined planes
                                 and the refined predicted IoUs take the first pass's place, so the filters, the NMS and `predicted_iou`,
                                 `stability_score`, `area`, `bbox`, `segmentation` describe the refined candidate; `point_coords` stays the grid
                                 point.  Composes with every option above (they all run behind it) and with multimask_output=False.  The second
                                 decode plan of a chunk holds ncand * points_per_batch pairs per image: the images (crops) decoded together are
                                 also bounded so that it stays at or below 1024 pairs (M2M_PAIRS_IN_FLIGHT; 5 images at the defaults).
    With use_m2m=False nothing of this runs: the path, the launches and the results are the ones above."""

    def __init__(self, model, points_per_side=32, points_per_batch=64, pred_iou_thresh=0.8, stability_score_thresh=0.95,
                 stability_score_offset=1.0, mask_threshold=0.0, box_nms_thresh=0.7, point_grids=None, multimask_output=True, max_candidates=None,
                 output_mode="binary_mask", crop_n_layers=0, min_mask_region_area=0, use_m2m=False):
        if crop_n_layers > 0:
            raise NotImplementedError("crop_n_layers > 0 is a per-call argument here: generate(image, crop_n_layers=...) / "
                                      "generate_batch(..., crop_n_layers=...), with crop_overlap_ratio, crop_n_points_downscale_factor, crop_nms_thresh")
        if min_mask_region_area > 0:
            raise NotImplementedError("min_mask_region_area > 0 is a per-call argument here: generate(image, min_mask_region_area=...) / "
                                      "generate_batch(..., min_mask_region_area=...), or amg_utils.postprocess_small_regions on a returned list")
        if use_m2m:
            raise NotImplementedError("use_m2m=True is a per-call argument here: generate(image, use_m2m=True) / generate_batch(..., use_m2m=True)")
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
        self.points_per_side = int(points_per_side) if point_grids is None else None
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
    def generate(self, image, min_mask_region_area=0, output_mode="binary_mask", crop_n_layers=0, crop_overlap_ratio=512 / 1500,
                 crop_n_points_downscale_factor=1, crop_nms_thresh=0.7, use_m2m=False):
        """image: RGB u8 [H, W, 3] (array or PIL) -> list of dicts.  The per-call options: see the class."""
        img = self.transforms._check_u8(image)
        return self.generate_batch([img], min_mask_region_area=min_mask_region_area, output_mode=output_mode, crop_n_layers=crop_n_layers,
                                   crop_overlap_ratio=crop_overlap_ratio, crop_n_points_downscale_factor=crop_n_points_downscale_factor,
                                   crop_nms_thresh=crop_nms_thresh, use_m2m=use_m2m)[0]

    def generate_batch(self, images, orig_hw=None, min_mask_region_area=0, output_mode="binary_mask", crop_n_layers=0, crop_overlap_ratio=512 / 1500,
                       crop_n_points_downscale_factor=1, crop_nms_thresh=0.7, use_m2m=False):
        """images: a list of RGB u8 [H, W, 3] images (orig_hw then defaults to their sizes), a [B, 3, R, R] tensor as `infer_masks` takes it, or
        the `Sam2Embeddings` `encode_images` made of one; orig_hw = [(H, W)] per image.  -> one list of dicts per image.  crop_n_layers > 0
        takes the list of u8 images only."""
        model = self.model
        if output_mode == "coco_rle":
            raise NotImplementedError("output_mode='coco_rle': the compressed string form is pycocotools', which is not available to check an "
                                      "encoder against; 'uncompressed_rle' carries the same runs")
        if output_mode not in ("binary_mask", "uncompressed_rle"):
            raise ValueError(f"output_mode must be 'binary_mask' or 'uncompressed_rle', not {output_mode!r}")
        min_area = int(min_mask_region_area)
        if min_area < 0:
            raise ValueError("min_mask_region_area must be >= 0")
        if int(crop_n_layers) < 0:
            raise ValueError("crop_n_layers must be >= 0")
        if int(crop_n_layers) > 0:
            return self._generate_batch_crops(images, int(crop_n_layers), float(crop_overlap_ratio), crop_n_points_downscale_factor,
                                              float(crop_nms_thresh), min_area, output_mode, bool(use_m2m))
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
        step = self._images_in_flight(bool(use_m2m))
        out = []
        for a in range(0, B, step):
            src = images[a:a + step]
            emb = src if isinstance(src, Sam2Embeddings) else model.encode_images(src)
            out += self._generate(emb, sizes[a:a + step], min_area, output_mode, bool(use_m2m))
        return out

    def _images_in_flight(self, m2m):
        """Images (or crops) per sub-batch: their candidate pools stay below POOL_BYTES_IN_FLIGHT and, with the mask-to-mask pass, the pairs of
        a chunk's second decode plan (ncand * points_per_batch per image) at or below M2M_PAIRS_IN_FLIGHT -- one image always goes through."""
        f0 = self.model.image_size // 4
        step = max(1, POOL_BYTES_IN_FLIGHT // (self.cap * f0 * f0 * 4))
        return min(step, max(1, M2M_PAIRS_IN_FLIGHT // (self.ncand * self.points_per_batch))) if m2m else step

    # -- one sub-batch
    def _candidates(self, emb, sizes, grid=None, points_in=None, crops=None, image_hw=None, m2m=False):
        """Enqueue every chunk of the grid for the images of `emb`: decode, score, filter + append.  -> the per-image device state
        (counter i32 [B, 2], records i32 [B, cap, 10], pool f32 [B, cap, R/4, R/4], block f32 [B, 5, cap]); nothing is read back.
        grid / points_in: a crop layer's grid in the place of the generator's; crops = [[x0, y0, x1, y1]] per "image" of `emb`, the crops of
        one image of size image_hw = (H, W): sizes are then the crops' and the append holds the border filter.
        m2m: every chunk's decode is `infer_masks(m2m=True)` -- the refined candidates and their predicted IoUs take the first pass's place
        in front of everything below, in the first pass's candidate order (so `point` and `token` name the first-pass candidate)."""
        lib, model = _lib.load(), self.model
        B, cap, C, Pb = len(emb), self.cap, self.ncand, self.points_per_batch
        f0 = model.image_size // 4
        lo, mid, hi = self.levels
        dev = emb.device
        grid = self.grid if grid is None else grid
        points_in = self.points_in if points_in is None else points_in
        sp = torch.cuda.current_stream().cuda_stream
        counter = torch.zeros(B, 2, dtype=torch.int32, device=dev)
        records = torch.zeros(B, cap, len(_lib.AMG_RECORD), dtype=torch.int32, device=dev)
        pool = torch.empty(B, cap, f0, f0, dtype=torch.float32, device=dev)
        block = torch.zeros(B, 5, cap, dtype=torch.float32, device=dev)
        block[:, 4].fill_(float("-inf"))                                         # unused columns never pass the NMS's conf_thres
        stats = torch.empty(B, Pb * C, 8, dtype=torch.int32, device=dev)
        labels = torch.ones(B, Pb, 1, dtype=torch.int32)
        m2m_kw = dict(m2m=True) if m2m else {}
        for base in range(0, len(grid), Pb):
            pts = points_in[base:base + Pb]
            n_valid = pts.shape[0]
            if n_valid < Pb:                                                     # a short last chunk: the last point repeated, never selected
                pts = torch.cat([pts, pts[-1:].expand(Pb - n_valid, 2)])
            _, low, iou = model.infer_masks(emb, points=pts.view(1, Pb, 1, 2).expand(B, Pb, 1, 2), point_labels=labels,
                                            multimask_output=self.multimask_output, return_high_res=False, **m2m_kw)
            low, iou = low.view(B, Pb * C, f0, f0), iou.view(B, Pb * C)
            for b, (H, W) in enumerate(sizes):
                _lib.check(lib.cvmi_amg_score(low[b].data_ptr(), Pb * C, f0, f0, H, W, lo, mid, hi, stats[b].data_ptr(), None, sp), "amg_score")
                args = (stats[b].data_ptr(), iou[b].data_ptr(), low[b].data_ptr(), Pb * C, n_valid * C, C, base, self.pred_iou_thresh,
                        self.stability_score_thresh, f0 * f0, cap, counter[b].data_ptr(), records[b].data_ptr(), pool[b].data_ptr(), block[b].data_ptr())
                if crops is None:
                    _lib.check(lib.cvmi_amg_select(*args, sp), "amg_select")
                else:
                    _lib.check(lib.cvmi_amg_select_crop(*args, *crops[b], image_hw[1], image_hw[0], CROP_EDGE_TOL, sp), "amg_select_crop")
        return dict(counter=counter, records=records, pool=pool, block=block)

    def _first_nms(self, st):
        """The per-image (per-crop) box NMS on a `_candidates` state and its results on their way to pinned memory, enqueued.
        -> (keep_idx on the device, the pinned buffers `_read` takes after the stream has been synchronised)."""
        lib, cap = _lib.load(), self.cap
        counter, records, block = st["counter"], st["records"], st["block"]
        B, dev = int(counter.shape[0]), counter.device
        max_det = min(cap, NMS_MAX_DET)
        ws = torch.empty(int(lib.cvmi_yolo_nms_workspace(B, cap)), dtype=torch.uint8, device=dev)
        det = torch.empty(B, max_det, 6, dtype=torch.float32, device=dev)
        keep_idx = torch.empty(B, max_det, dtype=torch.int32, device=dev)
        keep_n = torch.empty(B, dtype=torch.int32, device=dev)
        _lib.check(lib.cvmi_yolo_nms(block.data_ptr(), B, 1, cap, self.pred_iou_thresh, self.box_nms_thresh, max_det, 0.0, det.data_ptr(),
                                     keep_idx.data_ptr(), keep_n.data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream), "yolo_nms")
        # counts, kept indices and records in pinned buffers: valid after one synchronise
        host = [torch.empty(t.shape, dtype=t.dtype, pin_memory=True) for t in (counter, keep_n, keep_idx, records)]
        for h, t in zip(host, (counter, keep_n, keep_idx, records)):
            h.copy_(t, non_blocking=True)
        return keep_idx, host

    def _read(self, host):
        """After the wait: (kept_n [B], kept_idx [B, max_det], records [B, cap]) on the host; too many kept candidates raise."""
        counts, kept_n, kept_idx, recs = (h.numpy() for h in host)
        recs = recs.view(_lib.AMG_RECORD).reshape(counts.shape[0], self.cap)
        if int(counts[:, 0].max()) > self.cap:
            raise RuntimeError(f"{int(counts[:, 0].max())} candidates passed the filters but max_candidates = {self.cap}: raise max_candidates "
                               "(or the thresholds)")
        return kept_n, kept_idx, recs

    @staticmethod
    def _dict(seg, r, grid, crop):
        """The output dict of record r of a crop [cx0, cy0, cw, ch] (the image: [0, 0, W, H]): box and point moved to the image."""
        cx0, cy0, cw, ch = crop
        x0, y0, x1, y1 = int(r["x0"]), int(r["y0"]), int(r["x1"]), int(r["y1"])
        gx, gy = grid[int(r["point"])]
        return {"segmentation": seg, "area": int(r["area"]), "bbox": [x0 + cx0, y0 + cy0, x1 - x0, y1 - y0], "predicted_iou": float(r["score"]),
                "point_coords": [[float(gx * cw + cx0), float(gy * ch + cy0)]], "stability_score": float(r["stability"]), "crop_box": [cx0, cy0, cw, ch]}

    def _generate(self, emb, sizes, min_area=0, output_mode="binary_mask", m2m=False):
        """Candidates, NMS, the single host wait, then the survivors' masks."""
        with torch.cuda.device(emb.device):
            st = self._candidates(emb, sizes, m2m=m2m)
            keep_idx, host = self._first_nms(st)
            torch.cuda.current_stream().synchronize()                                # the one wait
            kept_n, kept_idx, recs = self._read(host)
            items = []
            for b, (H, W) in enumerate(sizes):
                K = int(kept_n[b])
                rows = [(recs[b, int(kept_idx[b, k])], self.grid, (0, 0, W, H)) for k in range(K)]
                items.append((H, W, st["pool"][b].index_select(0, keep_idx[b, :K].long()), rows) if K else None)
            if min_area > 0 or output_mode != "binary_mask":
                return self._finish_with_options(items, min_area, output_mode, self.box_nms_thresh)
            return [self._finish(item) for item in items]

    def _finish(self, item):
        """The dicts of one image's survivors (H, W, low planes [K, R/4, R/4], rows = [(record, grid, crop)]) with binary masks."""
        if item is None:
            return []
        H, W, low, rows = item
        masks = self._masks(low, H, W, [crop for _, _, crop in rows])
        return [self._dict(masks[k], r, grid, crop) for k, (r, grid, crop) in enumerate(rows)]

    # -- crop layers
    def _generate_batch_crops(self, images, n_layers, overlap_ratio, downscale, crop_nms_thresh, min_area, output_mode, m2m=False):
        if not isinstance(images, (list, tuple)):
            raise ValueError("crop_n_layers > 0 needs the pixels: images must be a list of RGB u8 images, not a tensor or embeddings")
        if self.points_per_side is None:
            raise ValueError("crop_n_layers > 0 with explicit point_grids (one grid): the layer grids come from points_per_side")
        grids = [(g, torch.from_numpy(g.astype(np.float32)) * float(self.model.image_size))
                 for g in amg_utils.build_all_layer_point_grids(self.points_per_side, n_layers, downscale)]
        imgs = [self.transforms._check_u8(im) for im in images]
        return [self._generate_crops(im, n_layers, overlap_ratio, grids, crop_nms_thresh, min_area, output_mode, m2m) for im in imgs]

    def _generate_crops(self, img, n_layers, overlap_ratio, grids, crop_nms_thresh, min_area, output_mode, m2m=False):
        """One image: its crops in sub-batches (one wait each), the cross-crop NMS (one wait), the survivors' masks in full-image planes."""
        from .detector import PackedImages
        model = self.model
        H, W = (int(v) for v in img.shape[:2])
        boxes, layers = amg_utils.generate_crop_boxes((H, W), n_layers, overlap_ratio)
        R, f0, cap = model.image_size, model.image_size // 4, self.cap
        packed = PackedImages.upload([img])                                       # the one H2D of the pixels
        step = self._images_in_flight(m2m)
        lows, rows = [], []
        for a in range(0, len(boxes), step):
            sub, n = boxes[a:a + step], len(boxes[a:a + step])
            x = torch.empty(n, R, R, 3, dtype=torch.float32, device=packed.data.device)
            # the crops are rows of one launch that share the image's offset: no cropped copy
            self.transforms._transform_srcs(PackedImages(packed.data, packed.offsets * n, packed.shapes * n), [tuple(c) for c in sub], x, F32, False)
            emb = model.encode_images(x.permute(0, 3, 1, 2))
            with torch.cuda.device(emb.device):
                groups, i = [], 0
                while i < n:                                                     # crops that share a layer grid are decoded together
                    j = i
                    while j < n and layers[a + j] == layers[a + i]:
                        j += 1
                    grid, points_in = grids[layers[a + i]]
                    st = self._candidates(emb[i:j], [(c[3] - c[1], c[2] - c[0]) for c in sub[i:j]], grid, points_in, sub[i:j], (H, W), m2m)
                    groups.append((i, j, grid, st["pool"], *self._first_nms(st)))
                    i = j
                torch.cuda.current_stream().synchronize()                        # the sub-batch's wait
                for i, j, grid, pool, keep_idx, host in groups:
                    kept_n, kept_idx, recs = self._read(host)
                    for b, c in enumerate(sub[i:j]):
                        K = int(kept_n[b])
                        if K:
                            lows.append(pool[b].index_select(0, keep_idx[b, :K].long()))
                            rows += [(recs[b, int(kept_idx[b, k])], grid, (c[0], c[1], c[2] - c[0], c[3] - c[1])) for k in range(K)]
        if not rows:
            return []
        low = torch.cat(lows)
        with torch.cuda.device(low.device):
            if len(boxes) > 1:
                order = self._cross_crop_nms(rows, crop_nms_thresh, low.device)
                rows = [rows[i] for i in order]
                low = low.index_select(0, torch.as_tensor(order, dtype=torch.long, device=low.device))
            item = (H, W, low, rows)
            if min_area > 0 or output_mode != "binary_mask":
                return self._finish_with_options([item], min_area, output_mode, max(self.box_nms_thresh, crop_nms_thresh))[0]
            return self._finish(item)

    def _cross_crop_nms(self, rows, nms_thresh, dev):
        """upstream's NMS across the crops: the boxes in image coordinates, score = 1 / (crop area) in f32 (a smaller crop wins; equal scores
        to the lower index).  One wait, for the keep list.  -> kept positions in NMS order."""
        lib, n = _lib.load(), len(rows)
        if n > NMS_MAX_DET:
            raise RuntimeError(f"{n} masks survived their crops' NMS but the NMS across the crops returns at most {NMS_MAX_DET}: raise the thresholds "
                               "(or lower crop_n_layers / points_per_side)")
        host = torch.empty(5, n, dtype=torch.float32, pin_memory=True)
        blk = host.numpy()
        for i, (r, _, (cx0, cy0, cw, ch)) in enumerate(rows):                    # halves of integers below 2^24: exact, as in cvmi_amg_select
            x0, y0, x1, y1 = int(r["x0"]) + cx0, int(r["y0"]) + cy0, int(r["x1"]) + cx0, int(r["y1"]) + cy0
            blk[:, i] = ((x0 + x1) / 2, (y0 + y1) / 2, x1 - x0, y1 - y0, np.float32(1.0) / np.float32(cw * ch))
        block = host.to(dev, non_blocking=True)
        ws = torch.empty(int(lib.cvmi_yolo_nms_workspace(1, n)), dtype=torch.uint8, device=dev)
        det = torch.empty(n, 6, dtype=torch.float32, device=dev)
        keep_idx = torch.empty(n, dtype=torch.int32, device=dev)
        keep_n = torch.empty(1, dtype=torch.int32, device=dev)
        _lib.check(lib.cvmi_yolo_nms(block.data_ptr(), 1, 1, n, 0.0, nms_thresh, n, 0.0, det.data_ptr(), keep_idx.data_ptr(), keep_n.data_ptr(),
                                     ws.data_ptr(), torch.cuda.current_stream().cuda_stream), "yolo_nms")
        keep_n, keep_idx = amg_utils._pinned(keep_n), amg_utils._pinned(keep_idx)
        torch.cuda.current_stream().synchronize()
        return keep_idx.numpy()[:int(keep_n[0])].tolist()

    # -- masks and the per-call options
    def _masks(self, low_planes, H, W, crops=None):
        """u8 [K, H, W] planes of the kept candidates' low-res planes, enqueued: cvmi_amg_score's mask mode, or -- for the planes of a crop
        [cx0, cy0, cw, ch] that is not the image -- cvmi_amg_score_window, which writes the crop's mask and the zeros around it in one pass.
        crops: one per plane; each run of planes of one crop is one call."""
        lib, f0 = _lib.load(), self.model.image_size // 4
        lo, mid, hi = self.levels
        K = int(low_planes.shape[0])
        masks = torch.empty(K, H, W, dtype=torch.uint8, device=low_planes.device)
        fstats = torch.empty(K, 8, dtype=torch.int32, device=low_planes.device)        # equal to the records' by construction; not read back
        sp = torch.cuda.current_stream().cuda_stream
        crops = [(0, 0, W, H)] * K if crops is None else crops
        a = 0
        while a < K:
            b = a + 1
            while b < K and crops[b] == crops[a]:
                b += 1
            cx0, cy0, cw, ch = crops[a]
            if (cx0, cy0, cw, ch) == (0, 0, W, H):
                _lib.check(lib.cvmi_amg_score(low_planes[a].data_ptr(), b - a, f0, f0, H, W, lo, mid, hi, fstats[a].data_ptr(), masks[a].data_ptr(), sp),
                           "amg_score")
            else:
                _lib.check(lib.cvmi_amg_score_window(low_planes[a].data_ptr(), b - a, f0, f0, ch, cw, lo, mid, hi, fstats[a].data_ptr(),
                                                     masks[a].data_ptr(), H, W, cx0, cy0, sp), "amg_score_window")
            a = b
        return masks

    def _finish_with_options(self, items, min_area, output_mode, nms_thresh):
        """After the first NMS's wait (and, with crops, the cross-crop NMS's): per image -- an item (H, W, low planes [K, R/4, R/4], rows =
        [(record, grid, crop)]) or None -- the survivors' planes (all of them, or chunk by chunk in the RLE mode), small-region removal, the
        second NMS with nms_thresh and the encoding are enqueued; ONE wait for all items; then the dicts."""
        rle = output_mode == "uncompressed_rle"
        work = []
        for item in items:
            if item is None:
                work.append(None)
                continue
            H, W, low, rows = item
            K = len(rows)
            crops = [crop for _, _, crop in rows]
            step = max(1, amg_utils.MASK_CHUNK_BYTES // (H * W)) if rle else K
            masks, infos, pending = None, [], []
            for a in range(0, K, step):
                def build(a=a, H=H, W=W, low=low, step=step, crops=crops):
                    m = self._masks(low[a:a + step], H, W, crops[a:a + step])
                    return m, (amg_utils.remove_small_enqueue(m, min_area, amg_utils.PHASES["both"]) if min_area > 0 else None)
                masks, info = build()
                infos.append(info)
                if rle:
                    pending.append(amg_utils.PendingRle(masks, rebuild=lambda build=build: build()[0]))
                    masks = None                                                 # the chunk's planes are free again once the stream has passed them
            nms = amg_utils.SecondNms(torch.cat(infos), nms_thresh) if min_area > 0 else None
            work.append((K, masks, pending, nms))
        torch.cuda.current_stream().synchronize()
        out = []
        for item, w in zip(items, work):
            if w is None:
                out.append([])
                continue
            rows = item[3]
            K, masks, pending, nms = w
            order, info = nms.finish() if nms is not None else (range(K), None)
            segs = [r for p in pending for r in p.finish()] if rle else masks
            dicts = []
            for k in order:
                d = self._dict(segs[k], *rows[k])
                dicts.append(amg_utils.survivor(d, segs[k], info[k]) if info is not None else d)
            out.append(dicts)
        return out
