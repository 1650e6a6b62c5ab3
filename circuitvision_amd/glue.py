"""The glue between the detector and the segmenter, on the device (cvmi_stage2_crop, csrc/glue_ops.hip).

What `CircuitPipeline` otherwise does on the host per chunk -- `detector.scale_boxes`, `pipeline.results_to_bboxes`' rounding,
`non_max_suppression_by_confidence`, `crop.crop_window`, `crop.adjust_bboxes` -- runs as ONE kernel on the detector's stream, on the detector
plan's own device outputs, and leaves the crop windows in device memory, where the segmenter's transform (`cvmi_sam2_transform_rects_dev`)
and mask post-processing (`cvmi_mask_postprocess_rects_dev`) read them.  The host is out of the chain: nothing between the detector's first
kernel and the segmenter's last depends on a value it has seen.

`to_host` builds, from the kernel's fixed-stride outputs and the detections' D2H copy, exactly the objects the host chain builds (bbox dicts
with their uid strings, the shifted list, the window tuple, `crop_debug_info`) -- after everything is enqueued, off the critical path.
The results are pinned bit for bit by tests/golden/nms_stage2.json and tests/golden/crop.json (tests/test_device_glue_gpu.py)."""
import struct

import numpy as np
import torch

from . import _lib
from .crop import _NOT_CLUSTERED, NON_COMPONENTS, _num

MAX_DET = 320                                   # include/cvmi355.h CVMI_GLUE_MAX_DET
INFO_HEAD = 40                                  # CVMI_GLUE_INFO_HEAD: words of the info record in front of the per-box words
FLAG_NOT_CLUSTERED, FLAG_JUNCTION, FLAG_TEXT, FLAG_NON_COMPONENT = 1, 2, 4, 8      # CVMI_GLUE_CLASS_*
BOX_EXPANDED, BOX_DROPPED = 1, 2                # CVMI_GLUE_BOX_*
# word indices of the info record (the enum in include/cvmi355.h)
(I_REASON, I_DECISION, I_APPLIED, I_LINK, I_CLUSTERS, I_MAIN_SIZE, I_MAIN_TEXT, I_MAIN_ID, I_MAIN_FIRST, I_TOTAL, I_COMPONENT_TYPE, I_TEXT_TYPE,
 I_PADDING, I_BASIS_SET, I_PADDED_SET, I_FINAL_SET) = range(16)
I_BASIS, I_PADDED, I_FINAL = 16, 24, 28
REASONS = (None, "no_elements_for_clustering", "crop_basis_bbox_too_large", "invalid_region_after_expansion")
DECISIONS = ("unknown", "no_crop_due_to_no_clustering_elements", "main_yolo_cluster_scored_by_text_assoc",
             "main_cluster_fallback_no_text_assoc_in_best_with_components")


def class_flags(names):
    """{class id: name} (or a list of names) -> uint8 [max id + 1]: what the crop asks of a class, by id (the sets of crop.py:19-20)."""
    items = dict(enumerate(names)) if isinstance(names, (list, tuple)) else {int(k): v for k, v in names.items()}
    out = np.zeros(max(items) + 1 if items else 0, dtype=np.uint8)
    for i, nm in items.items():
        out[i] = ((FLAG_NOT_CLUSTERED if nm in _NOT_CLUSTERED else 0) | (FLAG_JUNCTION if nm == "junction" else 0) |
                  (FLAG_TEXT if nm == "text" else 0) | (FLAG_NON_COMPONENT if nm in NON_COMPONENTS else 0))
    return out


class GlueOutputs:
    """The device tensors of one cvmi_stage2_crop launch (layouts: include/cvmi355.h)."""
    FIELDS = ("kept_idx", "kept_count", "boxes", "adj_boxes", "window", "info")

    def __init__(self, B, max_det, device, pinned=False):
        kw = dict(dtype=torch.int32, pin_memory=True) if pinned else dict(dtype=torch.int32, device=device)
        self.B, self.max_det = B, max_det
        self.kept_idx = torch.empty(B, max_det, **kw)
        self.kept_count = torch.empty(B, **kw)
        self.boxes = torch.empty(B, max_det, 4, **kw)
        self.adj_boxes = torch.empty(B, max_det, 4, **kw)
        self.window = torch.empty(B, 4, **kw)
        self.info = torch.empty(B, INFO_HEAD + max_det, **kw)

    def to_pinned(self):
        """Pinned host copies, enqueued on the current stream (non-blocking): valid once an event recorded after this call has completed."""
        h = GlueOutputs(self.B, self.max_det, None, pinned=True)
        for f in self.FIELDS:
            getattr(h, f).copy_(getattr(self, f), non_blocking=True)
        return h


def letterbox_scalars(lb_shape, orig_shape):
    """gain, pad_x, pad_y exactly as detector.scale_boxes computes them."""
    gain = min(lb_shape[0] / orig_shape[0], lb_shape[1] / orig_shape[1])
    return gain, round((lb_shape[1] - orig_shape[1] * gain) / 2 - 0.1), round((lb_shape[0] - orig_shape[0] * gain) / 2 - 0.1)


def stage2_crop(det, count, lb_shape, orig_shape, flags, padding, stage2_iou):
    """det f32 [B, max_det, 6] and count i32 [B] on the device (a detector plan's outputs, letterboxed coordinates), flags a DEVICE uint8
    tensor of class_flags -> GlueOutputs, enqueued on the current stream.  stage2_iou None or < 0: no stage-2 pass, list order."""
    lib = _lib.load()
    if not (torch.is_tensor(det) and det.is_cuda and det.dtype == torch.float32 and det.dim() == 3 and det.shape[2] == 6 and det.is_contiguous()):
        raise TypeError("stage2_crop expects a contiguous float32 [B, max_det, 6] device tensor")
    if not (torch.is_tensor(count) and count.is_cuda and count.dtype == torch.int32 and count.numel() == det.shape[0] and count.is_contiguous()):
        raise TypeError("stage2_crop expects an int32 [B] device tensor of counts")
    if not (torch.is_tensor(flags) and flags.is_cuda and flags.dtype == torch.uint8 and flags.is_contiguous()):
        raise TypeError("stage2_crop expects the class flags as a uint8 device tensor (upload class_flags(names) once)")
    B, max_det = det.shape[:2]
    gain, pad_x, pad_y = letterbox_scalars(lb_shape, orig_shape)
    out = GlueOutputs(B, max_det, det.device)
    _lib.check(lib.cvmi_stage2_crop(det.data_ptr(), count.data_ptr(), B, max_det, int(orig_shape[0]), int(orig_shape[1]), gain, pad_x, pad_y,
                                    -1.0 if stage2_iou is None else float(stage2_iou), int(padding), flags.data_ptr(), flags.numel(),
                                    out.kept_idx.data_ptr(), out.kept_count.data_ptr(), out.boxes.data_ptr(), out.adj_boxes.data_ptr(),
                                    out.window.data_ptr(), out.info.data_ptr(), torch.cuda.current_stream().cuda_stream), "stage2_crop")
    return out


# ---- the info record <-> crop_debug_info ---------------------------------------------------------------------------------------------------
def _f64_words(v):
    lo, hi = struct.unpack("<ii", struct.pack("<d", float(v)))
    return lo, hi


def _f64_from(lo, hi):
    return struct.unpack("<d", struct.pack("<ii", int(lo), int(hi)))[0]


def encode_info(info, bboxes):
    """crop_debug_info of crop.crop_window(bboxes, ..) -> the kernel's info record, int32 [INFO_HEAD + len(bboxes)] (the inverse of
    decode_info: what the kernel writes, stated on the host)."""
    rec = np.zeros(INFO_HEAD + len(bboxes), dtype=np.int32)
    rec[I_REASON] = REASONS.index(info["reason_for_no_crop"])
    rec[I_DECISION] = DECISIONS.index(info["crop_decision_source"])
    rec[I_APPLIED] = int(info["crop_applied"])
    rec[I_LINK] = -1 if info["clustering_proximity_threshold"] is None else info["clustering_proximity_threshold"]
    rec[I_CLUSTERS] = -1 if info["num_clusters_found"] is None else info["num_clusters_found"]
    mc = info["main_cluster_info"]
    rec[I_MAIN_FIRST] = -1
    if mc is not None:
        rec[I_MAIN_SIZE], rec[I_MAIN_TEXT], rec[I_MAIN_ID] = mc["num_elements"], mc["text_assoc_count"], mc["id"]
        rec[I_MAIN_FIRST] = next(k for k, b in enumerate(bboxes) if b.get("class") not in _NOT_CLUSTERED and b.get("persistent_uid") == mc["example_uid"])
    rec[I_TOTAL], rec[I_COMPONENT_TYPE], rec[I_TEXT_TYPE] = info["num_total_yolo_bboxes"], info["num_component_type_bboxes"], info["num_text_type_bboxes"]
    rec[I_PADDING] = info["padding_value"]
    if info["crop_basis_bbox_before_padding"] is not None:
        rec[I_BASIS_SET] = 1
        for c, v in enumerate(info["crop_basis_bbox_before_padding"]):
            rec[I_BASIS + 2 * c], rec[I_BASIS + 2 * c + 1] = _f64_words(v)
    for key, flag, at in (("window_after_main_padding", I_PADDED_SET, I_PADDED), ("final_crop_window_abs", I_FINAL_SET, I_FINAL)):
        if info[key] is not None:
            rec[flag] = 1
            rec[at:at + 4] = info[key]
    k = 0                                            # the entries are in list order: each is the next text box with its uid and coordinates
    for t in info["text_bboxes_that_expanded_crop"]:
        while not (bboxes[k].get("class") == "text" and bboxes[k].get("persistent_uid") == t["uid"] and
                   (bboxes[k]["xmin"], bboxes[k]["ymin"], bboxes[k]["xmax"], bboxes[k]["ymax"]) == tuple(t["coords_original"])):
            k += 1
        rec[INFO_HEAD + k] = BOX_EXPANDED
        k += 1
    return rec


def decode_info(rec, bboxes, image_hw):
    """One image's info record (sequence of INFO_HEAD + n ints) + the boxes the crop saw -> the crop_debug_info dict of crop.crop_window."""
    H, W = int(image_hw[0]), int(image_hw[1])
    rec = rec.tolist() if hasattr(rec, "tolist") else list(rec)
    applied = bool(rec[I_APPLIED])
    main = None
    if rec[I_MAIN_FIRST] >= 0:
        main = {"num_elements": rec[I_MAIN_SIZE], "text_assoc_count": rec[I_MAIN_TEXT], "score": (rec[I_MAIN_TEXT], rec[I_MAIN_SIZE]), "id": rec[I_MAIN_ID],
                "example_uid": bboxes[rec[I_MAIN_FIRST]].get("persistent_uid")}
    basis = tuple(_num(_f64_from(rec[I_BASIS + 2 * c], rec[I_BASIS + 2 * c + 1])) for c in range(4)) if rec[I_BASIS_SET] else None
    final = tuple(rec[I_FINAL:I_FINAL + 4]) if rec[I_FINAL_SET] else None
    grown = []
    for k, b in enumerate(bboxes):
        if rec[INFO_HEAD + k] & BOX_EXPANDED:
            xy = (b["xmin"], b["ymin"], b["xmax"], b["ymax"])
            grown.append({"uid": b.get("persistent_uid"), "class": b.get("class"), "coords_original": xy, "coords_text_box_abs": tuple(float(v) for v in xy)})
    return {"crop_applied": applied, "reason_for_no_crop": REASONS[rec[I_REASON]], "original_image_dims": (W, H),
            "num_total_yolo_bboxes": rec[I_TOTAL], "num_component_type_bboxes": rec[I_COMPONENT_TYPE], "num_text_type_bboxes": rec[I_TEXT_TYPE],
            "clustering_proximity_threshold": None if rec[I_LINK] < 0 else rec[I_LINK], "num_clusters_found": None if rec[I_CLUSTERS] < 0 else rec[I_CLUSTERS],
            "main_cluster_info": main, "crop_decision_source": DECISIONS[rec[I_DECISION]], "crop_basis_bbox_before_padding": basis,
            "padding_value": rec[I_PADDING], "window_after_main_padding": tuple(rec[I_PADDED:I_PADDED + 4]) if rec[I_PADDED_SET] else None,
            "text_bboxes_that_expanded_crop": grown, "final_crop_window_abs": final,
            "cropped_image_dims": (final[2] - final[0], final[3] - final[1]) if applied else (W, H)}


def to_host(det, count, out, names, orig_shape, uids=None):
    """The host chain's objects from the kernel's outputs.  det f32 [B, max_det, 6] and count: the detector's raw (letterboxed) detections --
    only their confidence and class columns are read; out: GlueOutputs (device tensors, or their pinned copies once complete).
    -> per image (bboxes: the stage-2 survivors as `results_to_bboxes` builds them, shifted: `adjust_bboxes` of them, window (x0, y0, x1, y1)
    or None, crop_debug_info).  uids: per image, a persistent_uid per DETECTOR box, for callers that carry ids of their own (default: the
    reference's class_x0_y0_x1_y1 string)."""
    host = lambda t: t.cpu() if t.is_cuda else t
    det_l = host(det)[:, :, 4:6]
    cnt = host(count).tolist()
    kept_n = host(out.kept_count).tolist()
    kept_idx, boxes, adj, info = host(out.kept_idx), host(out.boxes), host(out.adj_boxes), host(out.info)
    res = []
    for b, K in enumerate(kept_n):
        n = cnt[b]
        conf = det_l[b, :n, 0].numpy().tolist()
        ids = det_l[b, :n, 1].numpy().tolist()
        xy = boxes[b, :n].tolist()
        rec = info[b, :INFO_HEAD + K].tolist()
        bbs = []
        for i in kept_idx[b, :K].tolist():
            x0, y0, x1, y1 = xy[i]
            nm = names[int(ids[i])]
            bbs.append({"class": nm, "_yolo_class_id_temp": int(ids[i]), "confidence": conf[i], "xmin": x0, "ymin": y0, "xmax": x1, "ymax": y1,
                        "persistent_uid": f"{nm}_{x0}_{y0}_{x1}_{y1}" if uids is None else uids[b][i]})
        shifted = []
        for k, (bb, (x0, y0, x1, y1)) in enumerate(zip(bbs, adj[b, :K].tolist())):
            if not rec[INFO_HEAD + k] & BOX_DROPPED:
                nb = dict(bb)
                nb["xmin"], nb["ymin"], nb["xmax"], nb["ymax"] = x0, y0, x1, y1
                shifted.append(nb)
        dbg = decode_info(rec, bbs, orig_shape)
        res.append((bbs, shifted, dbg["final_crop_window_abs"] if dbg["crop_applied"] else None, dbg))
    return res
