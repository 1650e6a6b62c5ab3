"""Batched detector -> segmenter pipeline over a shard of circuit images (BASELINE configs[3]).

What it restates, batched and on the device, is the chain the reference runs per uploaded image:

    run_initial_detection              /root/reference/src/analysis_pipeline.py:97-115
        CircuitAnalyzer.bboxes         src/circuit_analyzer.py:267-287   (YOLO.predict -> dicts, python round(), persistent uid)
        non_max_suppression_by_confidence(iou 0.6)                       src/utils.py:346-361
    run_segmentation_and_cropping      src/analysis_pipeline.py:168-225
        crop_image_and_adjust_bboxes   src/circuit_analyzer.py:937-1284  (`crop=True`: this package's mirror, crop.py, padding 80 as at
                                                                          analysis_pipeline.py:177 -- the window is decided on the host
                                                                          from <= 300 boxes and handed to the segmenter's transform as a
                                                                          source rectangle of the u8 image already in HBM; `crop_fn`: any
                                                                          other callable with the reference's signature)
        CircuitAnalyzer.segment_with_sam2                                src/circuit_analyzer.py:321-386

`prompts="learned"` is the reference's own segmentation (one mask per image from the wrapper's learned prompts);
`prompts="boxes"` feeds the detector's boxes to `infer_masks(images, boxes)` (upstream box prompting, BASELINE configs[4]):
one mask per detected component; `prompts="both"` returns the two from one `encode_images` per chunk (`Sam2Embeddings`: the trunk runs once, the
learned-prompt decode and the box decode read its embeddings).

Images are independent through both models, so a batch shards contiguously over ranks with no collective on the data path
(`shard_range`); every rank returns the results of its own images, `gather_results` collects them on one rank when a single
caller needs them.  Results do not depend on how the batch is split (tests: sharded == unsharded, bit for bit).
"""
import time
from collections import defaultdict

import numpy as np
import torch

from .crop import adjust_bboxes, crop_image_and_adjust_bboxes, crop_window
from .detector import non_max_suppression_by_confidence
from .distributed import gather_rows, shard_range


def results_to_bboxes(r):
    """circuit_analyzer.py:267-287 on one `Results`: lists via .cpu().numpy().tolist(), python round() (half-to-even), uid string.
    (The four `round()` per box run as ONE np.rint over the float64 copy of the coordinates: the same half-to-even rounding of the same doubles.)"""
    ids = r.boxes.cls.cpu().numpy().tolist()
    conf = r.boxes.conf.cpu().numpy().tolist()
    xy = np.rint(r.boxes.xyxy.cpu().numpy().astype(np.float64)).astype(np.int64).tolist()
    names = r.names
    out = []
    for i, (x0, y0, x1, y1) in enumerate(xy):
        nm = names[int(ids[i])]
        out.append({"class": nm, "_yolo_class_id_temp": int(ids[i]), "confidence": conf[i], "xmin": x0, "ymin": y0, "xmax": x1, "ymax": y1,
                    "persistent_uid": f"{nm}_{x0}_{y0}_{x1}_{y1}"})
    return out


class CircuitPipeline:
    """detector: `circuitvision_amd.detector.YOLO`-like (`predict(list of uint8 HxWx3) -> [Results]`);
    segmenter: `SAM2Model`-like (`infer_masks(x, boxes=None)`, `.image_size`); transforms: `SAM2Transforms`-like."""

    def __init__(self, detector, segmenter, transforms, stage2_iou=0.6, max_prompts=32, crop_fn=None, swap_channels=True, seg_batch=16, crop=False,
                 crop_padding=80, nodes=False, reclassify=False, device_glue=False, mixed_batch=False):
        """crop=True: the reference's chain -- detector -> stage-2 NMS -> crop window from the boxes (crop.py) -> segmenter on the window
        (analysis_pipeline.py:177 -> :206); False: the segmenter sees the whole image.  crop_fn overrides the built-in crop.
        swap_channels: segment_with_sam2 applies cv2.COLOR_BGR2RGB to whatever it is given (circuit_analyzer.py:343), and the
        pipeline hands it RGB (analysis_pipeline.py:199-203) -- i.e. the reference's segmenter sees the channels reversed.
        seg_batch: images per segmenter launch (BASELINE configs[2] runs SAM 2.1-L at 16).
        max_prompts (prompts="boxes"): boxes per image handed to the segmenter; longer lists are cut, shorter ones filled with their first box (the
        tensor form `boxes[B,P,4]`).  None: every image's whole stage-2 box list as its own prompt list (`infer_masks` with lists: the decoder runs
        on the boxes there are, an image without boxes returns no mask).
        nodes=True (prompts="learned" or "both"): each result also carries get_node_connections' front end on its mask and boxes
        (circuit_analyzer.py:1325-1365, wires.node_contours): "emptied_mask", "resized_bboxes", "enhanced", "contours".
        nodes="connections" (prompts="learned" or "both"): get_node_connections through to its node list (:1325-1583, wires.node_connections):
        the keys of nodes=True plus "nodes" and "connection_points".
        reclassify=True (any prompts mode): run_terminal_reclassification (analysis_pipeline.py:117-137, wires.reclassify_terminals) runs
        after the segmenter and before node analysis, on the image the segmenter saw and its boxes, with the detector's names: a 'terminal'
        box that touches two or more wire contours becomes 'voltage.dc'.  "bboxes" are the rewritten boxes (node analysis reads them) and
        each result gains "terminal_connections": {box index: connected contours}.
        device_glue=True (needs crop=True without a crop_fn, and this package's own detector / segmenter / transforms): what sits between the
        two models in the cropped chain -- scale_boxes, rounding, stage-2 NMS, the crop window, the box shift -- runs as one kernel on the
        detector's stream (glue.py) and the segmenter reads its windows from device memory: no host wait between the detector's first kernel
        and the segmenter's last.  Same result dicts, key for key and bit for bit.
        mixed_batch=True: images of different sizes go to the detector as ONE batch (ultralytics' rule for a mixed list: every image
        letterboxed to the full imgsz x imgsz square, `YOLO.predict`) -- one packed upload, one ragged letterbox launch and one square plan per
        chunk size instead of a detector batch, a staging buffer and a plan per image size; the cropped chain's segmenter and `reclassify`
        read their windows out of the packed block.  False (default): one detector batch per image size, each on its own rectangle.  Not
        with device_glue=True: cvmi_stage2_crop takes one image size per launch."""
        if not (isinstance(nodes, bool) or nodes == "connections"):
            raise ValueError("nodes must be False, True or 'connections'")
        self.det, self.seg, self.tr = detector, segmenter, transforms
        self.device_glue = bool(device_glue)
        if self.device_glue and not (crop and crop_fn is None and self._product_objects()):
            raise ValueError("device_glue=True needs crop=True, no crop_fn, and this package's own YOLO / SAM2Model / SAM2Transforms")
        self.mixed_batch = bool(mixed_batch)
        if self.mixed_batch and self.device_glue:
            raise ValueError("mixed_batch=True cannot be combined with device_glue=True: the device glue takes one image size per launch")
        self._glue_flags = None                    # (class names, their flag table on the device)
        self.stage2_iou, self.max_prompts, self.swap = stage2_iou, max_prompts, swap_channels
        self.crop_padding = int(crop_padding)
        self.builtin_crop = bool(crop) and crop_fn is None
        self.crop_fn = crop_fn if crop_fn is not None else ((lambda im, bb: crop_image_and_adjust_bboxes(im, bb, padding=self.crop_padding)) if crop else None)
        self.seg_batch = max(1, int(seg_batch))
        self.seg_slots = 2                         # segmenter plan instances (each with its own stream) the overlapped path alternates between
        self.nodes = bool(nodes)
        self.node_connections = nodes == "connections"
        self.reclassify = bool(reclassify)
        self.timings = defaultdict(float)          # wall seconds per phase, accumulated over calls (bench.py prints them per step)

    def _tick(self, name, t0):
        t1 = time.perf_counter()
        self.timings[name] += t1 - t0
        return t1

    def _detector_groups(self, images):
        """Image indices per detector batch: one batch per image size, or -- mixed_batch=True -- the whole list as one."""
        if self.mixed_batch:
            return [list(range(len(images)))]
        groups = {}
        for i, im in enumerate(images):
            groups.setdefault(im.shape[:2], []).append(i)
        return list(groups.values())

    # ---- stage A: analysis_pipeline.py:97-115
    def detect(self, images):
        """-> per image: the bboxes that survive the second-stage NMS (list of dicts, original pixel coordinates)."""
        out = [None] * len(images)
        for idxs in self._detector_groups(images):                     # one detector batch per image size (mixed_batch: one in all)
            t = time.perf_counter()
            res = self.det.predict([images[i] for i in idxs], verbose=False)
            t = self._tick("detect.predict (H2D + letterbox + YOLO11 + NMS + D2H)", t)
            for i, r in zip(idxs, res):
                out[i] = non_max_suppression_by_confidence(results_to_bboxes(r), iou_threshold=self.stage2_iou)
            self._tick("detect.glue (dicts + round + uid + stage-2 NMS)", t)
        return out

    # ---- stage B: analysis_pipeline.py:168-225
    def segment(self, images, bboxes, prompts="learned"):
        """prompts="both": per chunk ONE `encode_images` and two decodes of its embeddings -- the learned-prompt mask ("mask", "extent", "iou", as
        "learned" returns them) and the per-box masks ("masks", "extents", "box_iou": what "boxes" returns as "masks", "extents", "iou")."""
        if prompts not in ("learned", "boxes", "both"):
            raise ValueError("prompts must be 'learned', 'boxes' or 'both'")
        crops, boxes_adj, infos = [], [], []
        for im, bb in zip(images, bboxes):
            info = None
            if self.crop_fn is not None:
                im, bb, info = self.crop_fn(im, [dict(b) for b in bb])
            crops.append(im)
            boxes_adj.append(bb)
            infos.append(info)
        out = []
        for c0 in range(0, len(crops), self.seg_batch):                   # one segmenter launch per seg_batch images
            sl = slice(c0, c0 + self.seg_batch)
            out += self._segment_chunk(crops[sl], boxes_adj[sl], prompts)
        for r, info in zip(out, infos):
            r["crop_debug_info"] = info
        return out

    def _product_objects(self):
        """True when detector / segmenter / transforms are this package's own classes (the stream-ordered fast paths use their internals);
        duck-typed stand-ins (tests, other back ends) take the generic path."""
        from .detector import YOLO
        from .sam2_infer import SAM2Model, SAM2Transforms
        return isinstance(self.det, YOLO) and isinstance(self.seg, SAM2Model) and isinstance(self.tr, SAM2Transforms)

    def _segment_chunk(self, crops, boxes_adj, prompts):
        t = time.perf_counter()
        if self._product_objects():
            x = self.tr.forward_batch(crops, swap_rb=self.swap)           # the BGR2RGB of circuit_analyzer.py:343 as a channel index on the device
        else:
            x = self.tr.forward_batch([np.ascontiguousarray(im[..., ::-1]) if self.swap else im for im in crops])
        t = self._tick("segment.transform (channel swap + H2D + resize / normalise)", t)
        if prompts == "both":                                            # the trunk once; both decodes read its embeddings
            x = self.seg.encode_images(x)
            t = self._tick("segment.encode_images (SAM 2.1 trunk + neck)", t)
            out = self._segment_chunk_learned(crops, boxes_adj, x, t)
            for r, rb in zip(out, self._segment_chunk_boxes(crops, boxes_adj, x, time.perf_counter())):
                r.update(masks=rb["masks"], extents=rb["extents"], box_iou=rb["iou"])
            return out
        return (self._segment_chunk_learned if prompts == "learned" else self._segment_chunk_boxes)(crops, boxes_adj, x, t)

    def _segment_chunk_learned(self, crops, boxes_adj, x, t):
        """x: the transformed images, or their embeddings."""
        out = []
        hi, lo, iou = self.seg.infer_masks(x)
        t = self._tick("segment.infer_masks (SAM 2.1 forward)", t)
        for b, im in enumerate(crops):
            u8, ext = self.tr.postprocess_to_mask(hi[b:b + 1], im.shape[:2])
            out.append({"image": im, "bboxes": boxes_adj[b], "mask": u8[0, 0], "extent": ext[0], "iou": iou[b]})
        self._tick("segment.postprocess (resize + threshold + u8 + extent + D2H of extents)", t)
        return out

    def _segment_chunk_boxes(self, crops, boxes_adj, x, t):
        R, out = self.seg.image_size, []
        if self.max_prompts is None:
            return self._segment_chunk_lists(crops, boxes_adj, x, t)
        P = self.max_prompts
        bx = torch.zeros(len(crops), P, 4)
        counts = []
        for b, (im, bb) in enumerate(zip(crops, boxes_adj)):
            bb = bb[:P]                                                  # already sorted by confidence (stage-2 NMS order)
            counts.append(len(bb))
            if bb:
                t_ = torch.tensor([[d["xmin"], d["ymin"], d["xmax"], d["ymax"]] for d in bb], dtype=torch.float32)
                t_ = self.tr.transform_boxes(t_, normalize=True, orig_hw=im.shape[:2]).reshape(-1, 4)
                bx[b, :len(bb)] = t_
                bx[b, len(bb):] = t_[0]                                  # unused prompt slots repeat the first box (results dropped)
            else:
                bx[b] = torch.tensor([0.0, 0.0, R, R])
        _, lo, iou = self.seg.infer_masks(x, bx, return_high_res=False)
        t = self._tick("segment.infer_masks (SAM 2.1 forward)", t)
        for b, im in enumerate(crops):
            k = counts[b]
            if k:
                u8, ext = self.tr.postprocess_to_mask(lo[b, :k].unsqueeze(0), im.shape[:2])
                masks, ext = u8[0], ext
            else:
                masks, ext = torch.zeros(0, *im.shape[:2], dtype=torch.uint8, device=lo.device), []
            out.append({"image": im, "bboxes": boxes_adj[b][:P], "masks": masks, "extents": ext, "iou": iou[b, :k]})
        self._tick("segment.postprocess (resize + threshold + u8 + extent + D2H of extents)", t)
        return out

    def _segment_chunk_lists(self, crops, boxes_adj, x, t):
        """max_prompts=None: every image's whole stage-2 box list goes to `infer_masks` as its own prompt list -- nothing cut, nothing repeated,
        no whole-image box for an image without boxes -- and the packed low-res planes are post-processed in one launch, each to the size of
        its image (`postprocess_to_masks_sized`)."""
        lists = []
        for im, bb in zip(crops, boxes_adj):
            t_ = torch.tensor([[d["xmin"], d["ymin"], d["xmax"], d["ymax"]] for d in bb], dtype=torch.float32).reshape(-1, 4)
            lists.append(self.tr.transform_boxes(t_, normalize=True, orig_hw=im.shape[:2]).reshape(-1, 4))
        counts = [int(l.shape[0]) for l in lists]
        if sum(counts) == 0:                                             # no box in the whole chunk: nothing to launch
            dev = x.device
            return [{"image": im, "bboxes": bb, "masks": torch.zeros(0, *im.shape[:2], dtype=torch.uint8, device=dev), "extents": [],
                     "iou": torch.zeros(0, device=dev)} for im, bb in zip(crops, boxes_adj)]
        _, lo, iou = self.seg.infer_masks(x, lists, return_high_res=False)
        t = self._tick("segment.infer_masks (SAM 2.1 forward)", t)
        base = getattr(lo[0], "_base", None)                             # the lists are `torch.split` views of one packed [N, h, w] block
        packed = base if base is not None and tuple(base.shape) == (sum(counts),) + tuple(lo[0].shape[1:]) else torch.cat(lo)
        sizes = [im.shape[:2] for im, k in zip(crops, counts) for _ in range(k)]
        planes, ext = self.tr.postprocess_to_masks_sized(packed.unsqueeze(1), sizes)
        boxes = self.tr.extents_to_boxes(ext)
        out, n0 = [], 0
        for b, (im, k) in enumerate(zip(crops, counts)):
            H, W = im.shape[:2]
            masks = planes[n0].as_strided((k, H, W), (H * W, W, 1)) if k else torch.zeros(0, H, W, dtype=torch.uint8, device=packed.device)
            out.append({"image": im, "bboxes": boxes_adj[b], "masks": masks, "extents": boxes[n0:n0 + k], "iou": iou[b]})
            n0 += k
        self._tick("segment.postprocess (resize + threshold + u8 + extent + D2H of extents)", t)
        return out

    def run_batch(self, images, prompts="learned", rank=0, world=1):
        """The share [lo, hi) of `images` that belongs to `rank`: detection, stage-2 NMS, (crop), segmentation.
        Returns [(global image index, result dict)]."""
        if self.nodes and prompts not in ("learned", "both"):
            raise ValueError("nodes=True needs prompts='learned' or 'both': node analysis reads the one mask per image of the learned prompts")
        lo, hi = shard_range(len(images), rank, world)
        mine = list(images[lo:hi])
        if not mine:
            return []
        if prompts == "learned" and self.builtin_crop and self._product_objects():
            res = self._run_cropped_dev(mine) if self.device_glue else self._run_cropped(mine)
        elif prompts == "learned" and self.crop_fn is None and self._product_objects():
            res = self._run_overlapped(mine)
        else:
            bboxes = self.detect(mine)
            res = self.segment(mine, bboxes, prompts)
            if self.reclassify:
                self._reclassify(res)
        if self.nodes:
            self._add_nodes(res)
        return [(lo + i, r) for i, r in enumerate(res)]

    # ---- run_terminal_reclassification (analysis_pipeline.py:117-137).  The image it is handed is the one the segmenter was handed; its
    #      BGR2RGB and the method's RGB2BGR cancel, so cvtColor(RGB2GRAY)'s R weight falls on channel 0 of that image.
    def _reclassify(self, res, src=None, windows=None):
        """res: result dicts of one chunk.  src / windows: the detector's u8 device block and the crop windows (the cropped chain), read in
        place; otherwise every r["image"] is uploaded."""
        from .wires import reclassify_terminals
        t = time.perf_counter()
        dev = self.seg.dev if hasattr(self.seg, "dev") else None
        with torch.cuda.device(dev if dev is not None else torch.cuda.current_device()):
            bbs = [r["bboxes"] for r in res]
            if src is not None:
                counts = reclassify_terminals(src, bbs, self.det.names, red_channel=0, windows=windows)
            else:
                counts = reclassify_terminals([r["image"] for r in res], bbs, self.det.names, red_channel=0)
        for r, c in zip(res, counts):
            r["terminal_connections"] = c
        self._tick("reclassify (segment_circuit + empty boxes + external contours + contour x terminal hits + class rewrite)", t)

    # ---- run_node_analysis (analysis_pipeline.py:227) -> get_node_connections up to get_contours (nodes=True) or to its node list
    #      (nodes="connections"), on the masks left on the device
    def _add_nodes(self, res):
        from .wires import node_connections, node_contours
        t = time.perf_counter()
        dev = self.seg.dev if hasattr(self.seg, "dev") else None
        with torch.cuda.device(dev if dev is not None else torch.cuda.current_device()):
            nodes = (node_connections if self.node_connections else node_contours)([r["mask"] for r in res], [r["bboxes"] for r in res])
        for r, n in zip(res, nodes):
            r.update(n)
        if self.node_connections:
            self._tick("nodes (empty boxes + resize + enhance_lines + external contours + D2H of the points + contour x box connections + node list)", t)
        else:
            self._tick("nodes (empty boxes + resize + enhance_lines + external contours + D2H of the points)", t)

    # ---- learned prompts, no crop: the segmenter does not depend on the detector's boxes (analysis_pipeline.py:168-225 passes the
    #      image, not the boxes, to segment_with_sam2), so the whole batch is ENQUEUED -- segmenter chunks on the segmenter's stream, the
    #      detector on its own -- and the host-side glue (D2H lists, round(), uid strings, stage-2 NMS) runs while the GPU works.
    def _run_overlapped(self, images):
        t = time.perf_counter()
        chunks = [images[c0:c0 + self.seg_batch] for c0 in range(0, len(images), self.seg_batch)]
        pend = [self._enqueue_learned(chunks[0], 0)]
        t = self._tick("enqueue: segmenter chunk 0 (stage u8 + H2D + transform + SAM 2.1 graph + post-process launches)", t)
        handles = [(idxs, self.det.predict_async([images[i] for i in idxs])) for idxs in self._detector_groups(images)]
        t = self._tick("enqueue: detector (stage u8 + H2D + letterbox + YOLO11 graph + NMS + D2H launches)", t)
        pend += [self._enqueue_learned(ch, (k + 1) % self.seg_slots) for k, ch in enumerate(chunks[1:])]
        t = self._tick("enqueue: segmenter chunks 1.. (same, while the GPU runs chunk 0)", t)
        bboxes = [None] * len(images)
        for idxs, h in handles:
            res = h.result()
            t = self._tick("wait: detector results on the host", t)
            for i, r in zip(idxs, res):
                bboxes[i] = non_max_suppression_by_confidence(results_to_bboxes(r), iou_threshold=self.stage2_iou)
            t = self._tick("detect.glue (dicts + round + uid + stage-2 NMS), overlapped with the segmenter", t)
        out, k = [], 0
        for ch, pd in zip(chunks, pend):
            u8s, exts, iou = pd()
            for b, im in enumerate(ch):
                out.append({"image": im, "bboxes": bboxes[k], "mask": u8s[b], "extent": exts[b], "iou": iou[b]})
                k += 1
        self._tick("wait: segmenter (GPU time not hidden behind host work) + extents to the host", t)
        if self.reclassify:
            self._reclassify(out)
        return out

    # ---- learned prompts WITH the reference's crop: the segmenter's input depends on the detector's boxes (analysis_pipeline.py:177 -> :206).
    #      What keeps the GPU busy across that dependency: the detector runs in chunks (one H2D for all images, a graph replay per chunk); as soon
    #      as chunk k's boxes are on the host, the glue + stage-2 NMS + crop window of its images run there and segmenter chunk k is enqueued --
    #      its transform reads each window out of the u8 block the detector's letterbox read -- while the GPU is still in detector chunks k + 1 ..
    #      and segmenter chunks < k.  Only chunk 0's detector pass + glue is not hidden.
    def _run_cropped(self, images):
        t = time.perf_counter()
        work = []                                                          # (image indices of the chunk, detector handle)
        for idxs in self._detector_groups(images):
            hs = self.det.predict_chunks_async([images[i] for i in idxs], self.seg_batch)
            work += [(idxs[k * self.seg_batch:(k + 1) * self.seg_batch], h) for k, h in enumerate(hs)]
        t = self._tick("enqueue: detector chunks (stage u8 + ONE H2D + per chunk: letterbox + YOLO11 graph + NMS + D2H launches)", t)
        out, pend = [None] * len(images), []
        for k, (idxs, h) in enumerate(work):
            res = h.result()
            t = self._tick("wait: detector chunk on the host" if k else "wait: detector chunk 0 on the host (not hidden: the segmenter needs its boxes)", t)
            wins, metas = [], []
            for i, r in zip(idxs, res):
                bb = non_max_suppression_by_confidence(results_to_bboxes(r), iou_threshold=self.stage2_iou)
                win, info = crop_window(bb, images[i].shape[:2], self.crop_padding)
                wins.append(win)
                metas.append((adjust_bboxes(bb, win), info))
            t = self._tick("glue (dicts + round + uid + stage-2 NMS + crop window + box shift)" + (", overlapped with the GPU" if k else ", chunk 0: not hidden"), t)
            pend.append((idxs, wins, metas, h.src, self._enqueue_learned(None, k % self.seg_slots, src=h.src, windows=wins, det_stream=self.det.stream)))
            t = self._tick("enqueue: segmenter chunk (transform from the windows of the detector's u8 block + SAM 2.1 graph + post-process)", t)
        for idxs, wins, metas, _src, fin in pend:
            u8s, exts, iou = fin()
            for b, i in enumerate(idxs):
                im, wnd = images[i], wins[b]
                view = im if wnd is None else im[wnd[1]:wnd[3], wnd[0]:wnd[2]]              # (a numpy view, as the reference's slice)
                out[i] = {"image": view, "bboxes": metas[b][0], "mask": u8s[b], "extent": exts[b], "iou": iou[b], "window": wnd,
                          "crop_debug_info": metas[b][1]}
        self._tick("wait: segmenter (GPU time not hidden behind host work) + extents to the host", t)
        if self.reclassify:                                                # the windows of the detector's u8 block, still in HBM
            for idxs, wins, _metas, src, _fin in pend:
                self._reclassify([out[i] for i in idxs], src=src, windows=wins)
        return out

    # ---- the same chain with the glue on the device (device_glue=True): per chunk the detector's stream carries letterbox + YOLO11 graph + NMS
    #      + the glue kernel (on the plan's own outputs, before the next replay overwrites them) + the D2H copies, and the segmenter's stream
    #      waits for THAT chunk's event -- not for the tail of the detector's stream -- then transforms from the windows in device memory.
    #      Everything is enqueued before the host waits for anything; building the dicts and uid strings happens behind the segmenter.
    def _run_cropped_dev(self, images):
        from . import glue
        t = time.perf_counter()
        names = self.det.names
        key = tuple(sorted(names.items()))
        if self._glue_flags is None or self._glue_flags[0] != key:
            self._glue_flags = (key, torch.from_numpy(glue.class_flags(names)).to(self.det.device))
        flags = self._glue_flags[1]

        def after(h):                                                      # on the detector's stream, right after the chunk's replay
            g = glue.stage2_crop(h.det_dev, h.cnt_dev, h.lb_shape, h.orig_shape, flags, self.crop_padding, self.stage2_iou)
            return g, g.to_pinned()
        groups = {}
        for i, im in enumerate(images):
            groups.setdefault(im.shape[:2], []).append(i)
        work = []
        for idxs in groups.values():
            hs = self.det.predict_chunks_async([images[i] for i in idxs], self.seg_batch, after_chunk=after)
            work += [(idxs[k * self.seg_batch:(k + 1) * self.seg_batch], h) for k, h in enumerate(hs)]
        t = self._tick("enqueue: detector chunks (stage u8 + ONE H2D + per chunk: letterbox + YOLO11 graph + NMS + glue kernel + D2H launches)", t)
        pend = [(idxs, h, self._enqueue_learned(None, k % self.seg_slots, src=h.src, windows=h.after[0].window, ready=h.done)) for k, (idxs, h) in enumerate(work)]
        t = self._tick("enqueue: segmenter chunks (wait for the chunk's event + transform from the device windows + SAM 2.1 graph + post-process)", t)
        out, rows = [None] * len(images), []
        for idxs, h, _fin in pend:
            h.done.synchronize()
            rows.append(glue.to_host(h.det, h.cnt, h.after[1], h.names, h.orig_shape))
        t = self._tick("glue readback (dicts + uid strings + crop_debug_info from the kernel's outputs), behind the segmenter", t)
        for (idxs, h, fin), chunk in zip(pend, rows):
            u8, exts, iou = fin()
            for b, i in enumerate(idxs):
                bbs, shifted, wnd, info = chunk[b]
                im = images[i]
                hh, ww = im.shape[:2] if wnd is None else (wnd[3] - wnd[1], wnd[2] - wnd[0])
                view = im if wnd is None else im[wnd[1]:wnd[3], wnd[0]:wnd[2]]
                out[i] = {"image": view, "bboxes": shifted, "mask": u8[b, :hh * ww].view(hh, ww), "extent": exts[b], "iou": iou[b], "window": wnd,
                          "crop_debug_info": info}
        self._tick("wait: segmenter (GPU time not hidden behind host work) + extents to the host", t)
        if self.reclassify:
            for (idxs, h, _fin), chunk in zip(pend, rows):
                self._reclassify([out[i] for i in idxs], src=h.src, windows=[r[2] for r in chunk])
        return out

    def _enqueue_learned(self, imgs, slot=0, src=None, windows=None, det_stream=None, ready=None):
        """transform -> SAM 2.1 (learned prompts) -> resize / threshold / u8 / extent for one chunk, enqueued on the stream of segmenter plan
        `slot` (consecutive chunks alternate between two plan instances on two streams: independent images, and two segmenter graphs side by
        side fill each other's kernel tails).  The chunk is `imgs` (host images), or the windows [(x0, y0, x1, y1) | None] of a u8 device block
        / PackedImages `src` (the cropped chain; ordered behind `det_stream` too), or -- device glue -- the windows of `src` that a DEVICE
        int32 [B, 4] {x0, y0, w, h} tensor names (glue.stage2_crop), ordered behind that chunk's event `ready` and not the tail of the detector's
        stream; its masks go to a fixed-stride u8 [B, H0 * W0] block (plane b holds its window's h * w pixels at its start), so no size or
        offset is needed on the host.  Returns a closure that waits for it: -> (u8 masks [H,W] per image -- or that block --, extent tuples,
        iou [B,1])."""
        seg, tr = self.seg, self.tr
        on_device = torch.is_tensor(windows)
        B = len(src) if src is not None else len(imgs)
        if on_device:
            sizes = None
        elif src is not None:                                           # windows of a u8 device block / PackedImages (the cropped chain)
            whole = src.shapes if hasattr(src, "shapes") else [tuple(src.shape[1:3])] * B
            sizes = [whole[b] if w is None else (w[3] - w[1], w[2] - w[0]) for b, w in enumerate(windows)]
        else:
            sizes = [tuple(im.shape[:2]) for im in imgs]
        with seg._lock, torch.cuda.device(seg.dev):
            p = seg.plan(B, slot=slot)
            sst = seg.slot_stream(slot)
            # outputs come from the CALLER's allocator pool; the segmenter's stream is ordered behind the caller's before it writes them
            iou = torch.empty_like(p.iou)
            ext = torch.empty(B, 4, dtype=torch.int32, device=seg.dev)
            ext_h = torch.empty(B, 4, dtype=torch.int32, pin_memory=True)
            if on_device:                                                   # one plane per H0 * W0 bytes
                stride = src.shape[1] * src.shape[2]
                u8 = u8s = torch.empty(B, stride, dtype=torch.uint8, device=seg.dev)
                planes = dict(window=windows, plane_stride=stride)
            elif all(sz == sizes[0] for sz in sizes):
                u8 = torch.empty(B, sizes[0][0], sizes[0][1], dtype=torch.uint8, device=seg.dev)
                u8s = [u8[b] for b in range(B)]
                planes = dict(orig_hw=sizes[0])
            else:                                                           # planes of different sizes, packed back to back: one launch
                offs = np.concatenate(([0], np.cumsum([h * w for h, w in sizes], dtype=np.int64)))
                u8 = torch.empty(int(offs[-1]), dtype=torch.uint8, device=seg.dev)
                u8s = [u8[int(offs[b]):int(offs[b + 1])].view(h, w) for b, (h, w) in enumerate(sizes)]
                planes = dict(sizes=sizes)
            sst.wait_stream(torch.cuda.current_stream())
            if on_device:
                sst.wait_event(ready)                                       # this chunk's detector pass + glue: not the tail of the detector's stream
            elif det_stream is not None:
                sst.wait_stream(det_stream)                                 # (the u8 block's H2D copy: already complete -- result() waited -- but stated)
            for t_ in (iou, ext, u8) + ((getattr(src, "data", src),) if src is not None else ()) + ((windows,) if on_device else ()):
                t_.record_stream(sst)                                       # written / read on sst: the allocator must not hand them out before sst is past them
            with torch.cuda.stream(sst):
                if src is not None:
                    tr.forward_windows(src, windows, swap_rb=self.swap, out=p.x_in.t, out_dtype=seg.dtype)
                else:
                    tr.forward_batch(imgs, swap_rb=self.swap, out=p.x_in.t, out_dtype=seg.dtype)
                p.plan.run()
                iou.copy_(p.iou, non_blocking=True)
                hi = p.high_res                                             # f32 [B,1,R,R]
                if tr.fills_small_regions:                                  # holes / sprinkles go while the logits are in HBM, before the resize
                    hi = tr.fill_small_regions(hi)
                    hi.record_stream(sst)
                tr.mask_return(hi, out=(u8, ext), **planes)
                ext_h.copy_(ext, non_blocking=True)
                done = torch.cuda.Event()
                done.record(sst)

        def finish():
            done.synchronize()
            return u8s, tr.extents_to_boxes(ext_h), iou
        return finish


def gather_results(results, key="mask", dst=0):
    """Collect one same-shaped tensor per image (e.g. the u8 mask of equally sized images) from every rank on `dst`:
    returns {global index: tensor} there, None elsewhere.  Shards may be uneven, and a rank may hold NO image (more ranks than
    images): it still enters the collectives -- with zero rows of the dtype / trailing shape the other ranks report -- instead
    of leaving them waiting."""
    import torch.distributed as dist
    local = [r[key] for _, r in results]
    multi = dist.is_initialized() and dist.get_world_size() > 1
    meta = (local[0].dtype, tuple(local[0].shape), str(local[0].device)) if local else None
    if multi:
        metas = [None] * dist.get_world_size()
        dist.all_gather_object(metas, meta)                                # every rank, before anything that could raise
        known = [m for m in metas if m is not None]
        if not known:
            return {} if dist.get_rank() == dst else None
        if any(m[:2] != known[0][:2] for m in known):
            raise ValueError(f"gather_results: ranks disagree on the dtype / shape of '{key}': {sorted(set(m[:2] for m in known), key=str)}")
        if meta is None:                                                   # empty shard: zero rows, on this rank's device
            dev = torch.device("cuda", torch.cuda.current_device()) if dist.get_backend() == "nccl" else torch.device("cpu")
            meta = (known[0][0], known[0][1], str(dev))
    elif meta is None:
        return {}
    dev = torch.device(meta[2])
    idx = torch.tensor([i for i, _ in results], dtype=torch.int64, device=dev)
    vals = torch.stack(local) if local else torch.zeros((0,) + meta[1], dtype=meta[0], device=dev)
    gi, gv = gather_rows(idx, dst), gather_rows(vals, dst)
    if gi is None:
        return None
    return {int(i): v for ids, vs in zip(gi, gv) for i, v in zip(ids.tolist(), vs)}
