"""References, seeded generators and named mutants for the detector's tail (op_matrix.NMS_ROWS / DECODE_ROWS; tests/test_detect_matrix_gpu.py).
CPU only: importing this module needs neither a GPU nor the library.

NMS.  The reference is oracle/nms.py::yolo_nms(return_indices=True), which restates ultralytics' non_max_suppression and torchvision's fp32 CPU
kernel; the comparison is exact (count, anchor indices, all six columns).  nms_inputs(row) builds [B, 4 + nc, A] predictions with EXACTLY row["n"]
best-class scores above conf_thres per image (and some at exactly conf_thres, which must not count).  nms_variant restates the same algorithm in
numpy with one deliberate mistake selected by mutant=; without a mutant it must equal the oracle on every row (tests/test_detect_ref_cpu.py).

Decode.  decode_ref is the fp64 statement of DFL expectation, dist2bbox, stride scale and sigmoid on inputs already rounded to the row's storage
type.  The kernel is held to |y - ref64| <= FACTOR (DEV_ABS + DEV_REL |ref64|) per family (box rows / class rows, per dtype), where DEV_ABS and DEV_REL
are the largest absolute and relative deviation of the fp32 statement (oracle.yolo11.Detect.decode) from fp64 over the family's rows, measured on
the CPU by `PYTHONPATH=. python tests/detect_ref.py` (from the repository root).  No kernel output enters these numbers."""
import functools
import zlib

import numpy as np
import torch

from oracle import nms as onms

TDT = {"f16": torch.float16, "f32": torch.float32}
STRIDES = (8.0, 16.0, 32.0)
SENTINEL = -12288.0

NMS_MUTANTS = ("conf_ge", "iou_ge", "ties_desc_anchor", "no_class_offset", "area_unoffset", "iou_fma", "max_det_off_by_one", "no_max_nms", "best_last_max")
DECODE_MUTANTS = ("best_last_max", "dfl_no_max", "anchor_no_half", "level_seam_off_by_one")

F32 = np.float32


def _seed(*parts):
    return zlib.crc32("/".join(str(p) for p in parts).encode())


# ================================================================ NMS: generators ================================================================
def _scores(g, row, A, n):
    """(candidate anchors [n], best score [A] f32): exactly n above conf_thres; of the others at least a third (>= 1) at exactly conf_thres."""
    conf = F32(row["conf"])
    perm = g.permutation(A)
    cand, non = perm[:n], perm[n:]
    best = np.zeros(A, F32)
    if row["equal_scores"]:
        best[cand] = F32(0.625)
    else:
        best[cand] = (conf + (F32(1) - conf) * g.uniform(0.05, 0.95, n).astype(F32)).astype(F32)
    at = max(1, len(non) // 3) if len(non) else 0
    best[non[:at]] = conf
    best[non[at:]] = (conf * g.uniform(0.0, 0.98, len(non) - at).astype(F32)).astype(F32)
    assert int((best > conf).sum()) == n and (len(non) == 0 or int((best == conf).sum()) >= 1), row["id"]
    return cand, best


def _class_rows(g, best, cls, nc, ties):
    """[nc, A] class scores whose first maximum is best[a] at class cls[a] -- or, with ties, at an earlier class where a second copy of the maximum
    is planted (about a tenth of the anchors)."""
    A = len(best)
    rows = (best[None, :] * g.uniform(0.0, 0.9, (nc, A)).astype(F32)).astype(F32)
    rows[cls, np.arange(A)] = best
    if ties and nc > 1:
        tie = g.random(A) < 0.1
        other = (cls + 1 + g.integers(0, nc - 1, A)) % nc
        rows[other[tie], np.arange(A)[tie]] = best[tie]
    return rows


def _cluster_boxes(g, row, A):
    K = row["clusters"]
    centre = g.uniform(50, 590, (K, 2)).astype(F32)
    size = g.uniform(30, 90, (K, 2)).astype(F32)
    if row["zero"]:
        nz = int(K * row["zero"])
        size[:nz] = 0                                                      # zero-area boxes, duplicated by every member of the cluster
        size[nz:nz + max(1, nz // 2), 0] = 0                               # zero width, positive height
    k = g.integers(0, K, A)
    xy = centre[k] + (g.normal(0, 1, (A, 2)) * row["jitter"]).astype(F32)
    wh = size[k] * (F32(1) + (g.normal(0, 0.013, (A, 2)) * row["jitter"]).astype(F32))
    cls = np.where(g.random(A) < 0.85, k % row["nc"], g.integers(0, row["nc"], A))
    return np.concatenate((xy, wh), 1).astype(F32), cls


def _isolated_boxes(g, row, A):
    i = np.arange(A)
    xy = np.stack(((i % 70) * 100 + 50, (i // 70) * 100 + 50), 1).astype(F32)
    wh = (40 + g.integers(-5, 6, (A, 2))).astype(F32)
    return np.concatenate((xy, wh), 1), g.integers(0, row["nc"], A)


def _touch_boxes(g, row, A):
    """Cells of three 20 x 20 integer boxes: [10, 30], [30, 50] (shares an edge with the first) and [20, 40] shifted down by 4 (overlaps both)."""
    i = np.arange(A)
    cell, m = i // 3, i % 3
    ox, oy = (cell % 30) * 200, (cell // 30) * 200
    cx = ox + np.choose(m, (20, 40, 30))
    cy = oy + np.choose(m, (20, 20, 24))
    return np.stack((cx, cy, np.full(A, 20), np.full(A, 20)), 1).astype(F32), np.zeros(A, np.int64)


def _clsoff_boxes(g, row, A):
    """Cells of four identical boxes under classes 61, 60, 0 and 61 again."""
    i = np.arange(A)
    cell, m = i // 4, i % 4
    base = np.stack(((cell % 20) * 150 + 75.5, (cell // 20) * 150 + 60.25, 40 + (cell % 7) * 3.5, 30 + (cell % 5) * 4.25), 1).astype(F32)
    return base, np.choose(m, (61, 60, 0, 61))


def iou32(bi, bj, off, fma=False, area_unoffset=False):
    """torchvision's fp32 IoU of the box pairs (bi[k], bj[k]) (xyxy f32, class offset off[k] added first), one rounding per operation.
    fma: the union as a compiler may contract it, (a_i + a_j) - w * h with the product unrounded.  area_unoffset: areas from the boxes before
    the offset is added."""
    bi, bj, off = bi.astype(F32), bj.astype(F32), off.astype(F32)[:, None]
    oi, oj = bi + off, bj + off
    si, sj = (bi, bj) if area_unoffset else (oi, oj)
    ai = (si[:, 2] - si[:, 0]) * (si[:, 3] - si[:, 1])
    aj = (sj[:, 2] - sj[:, 0]) * (sj[:, 3] - sj[:, 1])
    w = np.maximum(F32(0), np.minimum(oi[:, 2], oj[:, 2]) - np.maximum(oi[:, 0], oj[:, 0]))
    h = np.maximum(F32(0), np.minimum(oi[:, 3], oj[:, 3]) - np.maximum(oi[:, 1], oj[:, 1]))
    inter = w * h
    assert inter.dtype == F32 and ai.dtype == F32
    if fma:
        union = ((ai + aj).astype(np.float64) - w.astype(np.float64) * h.astype(np.float64)).astype(F32)     # (the f64 product of two f32 is exact)
    else:
        union = (ai + aj) - inter
    with np.errstate(all="ignore"):
        return inter / union


def _xyxy32(b):
    hw, hh = b[:, 2] / F32(2), b[:, 3] / F32(2)
    return np.stack((b[:, 0] - hw, b[:, 1] - hh, b[:, 0] + hw, b[:, 1] + hh), 1).astype(F32)


def _iou64(bi, bj):
    bi, bj = bi.astype(np.float64), bj.astype(np.float64)
    w = np.maximum(0, np.minimum(bi[:, 2], bj[:, 2]) - np.maximum(bi[:, 0], bj[:, 0]))
    h = np.maximum(0, np.minimum(bi[:, 3], bj[:, 3]) - np.maximum(bi[:, 1], bj[:, 1]))
    a = lambda b: (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    return w * h / (a(bi) + a(bj) - w * h)


ROUNDING_SEARCH = 200000           # seeded pairs the class-offset search looks at
ROUNDING_CLASS = 61                # offset 61 * 7680 = 468480: one fp32 step is 1/32 pixel there
ROUNDING_PICK = 24                 # pairs of each family in the row
ROUNDING_FOUND = {"offset": 3762, "fma": 233}      # what the two searches find (tests/test_detect_ref_cpu.py holds them to it)


def _pair_grid(g, N):
    """N shifted box pairs (xywh f32) with IoU = thr (1 + O(2 %)), each in one of 18 x 18 cells of 400 px."""
    cell = g.integers(0, 324, N)
    xy = np.stack(((cell % 18) * 400, (cell // 18) * 400), 1) + g.uniform(100, 300, (N, 2))
    wh = g.uniform(20, 120, (N, 2))
    return cell, np.concatenate((xy, wh), 1).astype(F32)


@functools.lru_cache(maxsize=None)
def offset_flips(iou_thres=0.7, max_wh=7680.0, N=ROUNDING_SEARCH):
    """Pairs at class ROUNDING_CLASS whose fp32, non-contracted verdict (the oracle's arithmetic) differs from the exact one (fp64 IoU of the same
    fp32 corner coordinates without the offset): (cell, box_i, box_j xywh, verdict32) of every flip among N seeded pairs."""
    g = np.random.default_rng(_seed("offset_flips"))
    cell, bi = _pair_grid(g, N)
    thr = F32(iou_thres)
    dx = bi[:, 2] * (1 - iou_thres) / (1 + iou_thres) * (1 + g.uniform(-0.02, 0.02, N))
    bj = bi.copy()
    bj[:, 0] = (bi[:, 0] + dx).astype(F32)
    v32 = iou32(_xyxy32(bi), _xyxy32(bj), np.full(N, F32(ROUNDING_CLASS) * F32(max_wh))) > thr
    v64 = _iou64(_xyxy32(bi), _xyxy32(bj)) > float(thr)
    f = np.nonzero(v32 != v64)[0]
    return cell[f], bi[f], bj[f], v32[f]


@functools.lru_cache(maxsize=None)
def fma_flips(iou_thres=0.7, N=40000):
    """Pairs at class 0 whose verdict differs between the non-contracted union and a contracted one.  For each seeded pair the shift is bisected
    in fp32 until the non-contracted IoU straddles the threshold between two neighbouring shifts; both neighbours are tried."""
    g = np.random.default_rng(_seed("fma_flips"))
    cell, bi = _pair_grid(g, N)
    thr, zero = F32(iou_thres), np.zeros(N, F32)
    xi = _xyxy32(bi)

    def pair(dx):
        bj = bi.copy()
        bj[:, 0] = bi[:, 0] + dx
        return bj

    lo, hi = np.zeros(N, F32), bi[:, 2].copy()                           # IoU(lo) = 1 > thr, IoU(hi) = 0
    for _ in range(40):
        mid = ((lo + hi) / F32(2)).astype(F32)
        above = iou32(xi, _xyxy32(pair(mid)), zero) > thr
        lo, hi = np.where(above, mid, lo), np.where(above, hi, mid)
    out = []
    for dx in (lo, hi):
        bj = pair(dx)
        plain = iou32(xi, _xyxy32(bj), zero) > thr
        f = np.nonzero(plain != (iou32(xi, _xyxy32(bj), zero, fma=True) > thr))[0]
        out.append((cell[f], bi[f], bj[f], plain[f]))
    return tuple(np.concatenate(c) for c in zip(*out))


def rounding_pairs():
    """The row's pairs: ROUNDING_PICK of each family in distinct cells, as (class, box_i, box_j, verdict of the fp32 non-contracted arithmetic)."""
    out = []
    for cls, (cell, bi, bj, v) in ((ROUNDING_CLASS, offset_flips()), (0, fma_flips())):
        seen, take = set(), []
        for k in range(len(cell)):
            if int(cell[k]) not in seen:
                seen.add(int(cell[k]))
                take.append(k)
            if len(take) == ROUNDING_PICK:
                break
        assert len(take) == ROUNDING_PICK, (cls, len(cell))
        out += [(cls, bi[k], bj[k], bool(v[k])) for k in take]
    return out


def _rounding_image(g, row, A):
    pairs = rounding_pairs()
    n = 2 * len(pairs)
    assert row["n"] == n and A >= n and F32(row["iou"]) == F32(0.7) and row["max_wh"] == 7680.0
    perm = g.permutation(A)
    box, _ = _cluster_boxes(g, dict(row, clusters=4, jitter=1.5), A)
    cls = g.integers(1, 60, A)
    best = (F32(row["conf"]) * g.uniform(0, 0.98, A).astype(F32)).astype(F32)
    best[perm[n]] = F32(row["conf"])
    for k, (c, bi, bj, _) in enumerate(pairs):
        i, j = perm[2 * k], perm[2 * k + 1]
        box[i], box[j], cls[i], cls[j] = bi, bj, c, c
        best[i], best[j] = F32(0.9 - 0.004 * k), F32(0.6 - 0.004 * k)     # box i is kept first and judges box j
    return box, cls, best


def _maxnms_image(g, row, A):
    assert A == row["n"] and A > 30000 + 100
    perm = g.permutation(A)
    rank = np.empty(A, np.int64)
    rank[perm] = np.arange(A)                                             # rank 0 = best score
    best = (F32(row["conf"]) + F32(0.74) * (F32(0.02) + (A - rank).astype(F32) / F32(A) * F32(0.96))).astype(F32)
    assert len(np.unique(best)) == A and float(best.min()) > row["conf"]
    k = g.integers(0, 40, A)
    xy = np.stack(((k % 8) * 300 + 150, (k // 8) * 300 + 150), 1) + g.uniform(-0.5, 0.5, (A, 2))
    box = np.concatenate((xy, np.full((A, 2), 100.0)), 1).astype(F32)
    cls = k % row["nc"]
    weak = perm[A - 100:]                                                 # the 100 weakest: isolated, 150 px apart, far below the clusters
    i = np.arange(100)
    box[weak] = np.stack(((i % 10) * 150 + 75, 4000 + (i // 10) * 150, np.full(100, 50), np.full(100, 50)), 1).astype(F32)
    return box, cls, best


def nms_inputs(row):
    """pred f32 [B, 4 + nc, A] of an NMS row, seeded by its id."""
    B, nc, A, n = row["B"], row["nc"], row["A"], row["n"]
    pred = np.zeros((B, 4 + nc, A), F32)
    for b in range(B):
        g = np.random.default_rng(_seed(row["id"], b))
        if row["kind"] == "rounding":
            box, cls, best = _rounding_image(g, row, A)
        elif row["kind"] == "maxnms":
            box, cls, best = _maxnms_image(g, row, A)
        else:
            box, cls = {"cluster": _cluster_boxes, "isolated": _isolated_boxes, "touch": _touch_boxes, "clsoff": _clsoff_boxes}[row["kind"]](g, row, A)
            _, best = _scores(g, row, A, n)
        pred[b, :4] = box.T
        pred[b, 4:] = _class_rows(g, best, np.asarray(cls), nc, ties=row["kind"] in ("cluster", "isolated"))
    assert ((pred[:, 4:].max(1) > F32(row["conf"])).sum(1) == n).all(), row["id"]
    return torch.from_numpy(pred)


@functools.lru_cache(maxsize=None)
def nms_case(rid):
    """(row, pred, reference detections, reference anchor indices) of an NMS row: computed once per process, shared, never modified."""
    from op_matrix import NMS_ROWS
    row = next(r for r in NMS_ROWS if r["id"] == rid)
    pred = nms_inputs(row)
    with np.errstate(all="ignore"):
        det, idx = onms.yolo_nms(pred, row["conf"], row["iou"], row["max_det"], max_wh=row["max_wh"], return_indices=True)
    return row, pred, det, idx


def best_of(pred):
    """(best score [B, A] f32, best class [B, A] i32): the first maximum, as cvmi_yolo_nms_best expects it from the decode kernel."""
    s, c = pred[:, 4:].max(1)
    return s.contiguous(), c.int().contiguous()


# ================================================================ NMS: the algorithm again, with mutants ==========================================
def nms_variant(pred, conf_thres, iou_thres, max_det, max_wh, max_nms=30000, mutant=None):
    """yolo_nms restated in numpy: (list of [k, 6] f32, list of [k] anchor indices).  mutant selects one deliberate mistake."""
    assert mutant is None or mutant in NMS_MUTANTS, mutant
    p = pred.numpy().astype(F32)
    conf, thr = F32(conf_thres), F32(iou_thres)
    dets, idxs = [], []
    for b in range(p.shape[0]):
        sc = p[b, 4:]
        nc = sc.shape[0]
        cls = nc - 1 - sc[::-1].argmax(0) if mutant == "best_last_max" else sc.argmax(0)
        best = sc.max(0)
        a = np.nonzero(best >= conf if mutant == "conf_ge" else best > conf)[0]
        if mutant == "ties_desc_anchor":
            a = a[::-1]
        a = a[np.argsort(-best[a], kind="stable")]
        if mutant != "no_max_nms":
            a = a[:max_nms]
        xyxy = _xyxy32(p[b, :4][:, a].T)
        off = (cls[a].astype(F32) * F32(max_wh))[:, None] * F32(0 if mutant == "no_class_offset" else 1)
        ob = (xyxy + off).astype(F32)
        src = xyxy if mutant == "area_unoffset" else ob
        area = ((src[:, 2] - src[:, 0]) * (src[:, 3] - src[:, 1])).astype(F32)
        n = len(a)
        supp = np.zeros(n, bool)
        keep = []
        with np.errstate(all="ignore"):
            for i in range(n):
                if supp[i]:
                    continue
                keep.append(i)
                r = slice(i + 1, n)
                w = np.maximum(F32(0), np.minimum(ob[i, 2], ob[r, 2]) - np.maximum(ob[i, 0], ob[r, 0]))
                h = np.maximum(F32(0), np.minimum(ob[i, 3], ob[r, 3]) - np.maximum(ob[i, 1], ob[r, 1]))
                inter = w * h
                if mutant == "iou_fma":
                    union = ((area[i] + area[r]).astype(np.float64) - w.astype(np.float64) * h.astype(np.float64)).astype(F32)
                else:
                    union = (area[i] + area[r]) - inter
                ovr = inter / union
                supp[r] |= (ovr >= thr) if mutant == "iou_ge" else (ovr > thr)
        keep = np.asarray(keep[:max_det - 1 if mutant == "max_det_off_by_one" else max_det], np.int64)
        k = a[keep]
        dets.append(torch.from_numpy(np.concatenate((xyxy[keep], best[k, None], cls[k, None].astype(F32)), 1).astype(F32).reshape(-1, 6)))
        idxs.append(torch.from_numpy(k.astype(np.int64)))
    return dets, idxs


def same_detections(a, b):
    """Exact equality of two (detections, indices) results: count, anchor indices and all six columns of every image."""
    return all(x.shape == y.shape and torch.equal(x, y) for x, y in zip(a[0], b[0])) and all(torch.equal(x, y) for x, y in zip(a[1], b[1]))


# ================================================================ decode ==========================================================================
def decode_inputs(row, dt):
    """[(box [B, h, w, 64], cls [B, h, w, nc]) per level] as f32 tensors whose values are already rounded to the storage type dt."""
    g = torch.Generator().manual_seed(_seed(row["id"], dt))
    B, nc, out = row["B"], row["nc"], []
    for h, w in row["levels"]:
        box = torch.randn(B, h, w, 64, generator=g) * 2
        cls = torch.randn(B, h, w, nc, generator=g) * 2
        if row["kind"] == "ties":                                          # half-integer logits: every anchor has several equal channels ...
            cls = (cls * 0.75).round() / 2
            cls[:, 0] = 1.5                                                # ... the first grid row holds one value in every channel ...
            cls[:, -1, :, nc // 2:] = 30.0                                 # ... and the last one saturates its upper half (sigmoid = 1 in fp32)
        elif row["kind"] == "saturated":
            pick = torch.randint(0, 5, box.shape, generator=g)
            box = torch.tensor([-1000.0, -30.0, 0.0, 30.0, 1000.0])[pick]
            pick = torch.randint(0, 5, cls.shape, generator=g)
            cls = torch.tensor([-1000.0, -20.0, 0.0, 20.0, 1000.0])[pick]
        out.append((box.to(TDT[dt]).float(), cls.to(TDT[dt]).float()))
    return out


def decode_ref(levels, dtype=torch.float64, mutant=None):
    """[B, 4 + nc, A]: softmax expectation over the 16 bins of each side, dist2bbox around the anchor centre (x + 0.5, y + 0.5), stride scale,
    class sigmoid.  mutant: one deliberate mistake (DECODE_MUTANTS; best_last_max belongs to best_ref)."""
    assert mutant is None or mutant in DECODE_MUTANTS, mutant
    bins = torch.arange(16, dtype=dtype)
    outs = []
    for l, (box, cls) in enumerate(levels):
        B, h, w, _ = box.shape
        v = box.to(dtype).view(B, h * w, 4, 16)
        if mutant == "dfl_no_max":
            e = torch.exp(v)
        else:
            e = torch.exp(v - v.amax(-1, keepdim=True))
        dist = (e * bins).sum(-1) / e.sum(-1)                               # [B, hw, 4]: left, top, right, bottom
        al = torch.arange(h * w)
        ax, ay, st = (al % w).to(dtype), (al // w).to(dtype), STRIDES[l]
        if mutant == "level_seam_off_by_one" and l > 0:                    # the level's first anchor is looked up in the level before it
            hp, wp = levels[l - 1][0].shape[1:3]
            ax[0], ay[0] = float((hp * wp) % wp), float((hp * wp) // wp)
            st = torch.full((h * w,), STRIDES[l], dtype=dtype)
            st[0] = STRIDES[l - 1]
        half = 0.0 if mutant == "anchor_no_half" else 0.5
        x1, y1, x2, y2 = ax + half - dist[..., 0], ay + half - dist[..., 1], ax + half + dist[..., 2], ay + half + dist[..., 3]
        xywh = torch.stack(((x1 + x2) / 2 * st, (y1 + y2) / 2 * st, (x2 - x1) * st, (y2 - y1) * st), 1)
        outs.append(torch.cat((xywh, torch.sigmoid(cls.to(dtype)).view(B, h * w, -1).transpose(1, 2)), 1))
    return torch.cat(outs, 2)


def decode_chain32(row, levels):
    """The fp32 statement: oracle.yolo11.Detect.decode on the same inputs."""
    from oracle.yolo11 import Detect
    head = Detect(row["nc"], (64, 128, 256)[:len(levels)]).eval()
    with torch.no_grad():
        return head.decode([torch.cat((box, cls), -1).permute(0, 3, 1, 2).contiguous() for box, cls in levels])


def best_ref(cls_rows, mutant=None):
    """(best score, best class) of class rows [B, nc, A]: the first maximum (mutant best_last_max: the last)."""
    if mutant == "best_last_max":
        s, c = cls_rows.flip(1).max(1)
        return s, cls_rows.shape[1] - 1 - c
    return cls_rows.max(1)


SATURATED_RANK = {-1000.0: 0, -20.0: 1, 0.0: 2, 20.0: 3, 1000.0: 3}


def decode_exact_cls(row, levels):
    """[B, A] best class of the tie rows, from the logits alone: the sigmoid is monotone, so the first maximum of the logits wins.  In the saturated
    row 20 and 1000 share a rank: sigmoid(20) is within 2.1e-9 of 1, a fifteenth of the fp32 step below 1, so both are exactly 1.0f."""
    assert row["kind"] in ("ties", "saturated"), row["id"]
    out = []
    for _, cls in levels:
        v = cls.reshape(cls.shape[0], -1, cls.shape[-1])
        if row["kind"] == "saturated":
            rank = torch.zeros_like(v)
            for val, r in SATURATED_RANK.items():
                rank[v == val] = r
            v = rank
        out.append(v.max(2).indices)
    return torch.cat(out, 1)


@functools.lru_cache(maxsize=None)
def decode_case(rid, dt):
    """(row, per-level inputs, ref64) of a decode row: computed once per process, shared, never modified."""
    from op_matrix import DECODE_ROWS
    row = next(r for r in DECODE_ROWS if r["id"] == rid)
    levels = decode_inputs(row, dt)
    return row, levels, decode_ref(levels)


# Class rows: |y - ref64| <= FACTOR (DEV_ABS + DEV_REL |ref64|), the fp32 statement's largest absolute and relative (over scores above 0) deviation
# from fp64 over the family's rows.  Box rows: |y - ref64| <= FACTOR DEV_S S, where S is the magnitude of the terms the value is made of --
# stride (anchor index + 0.5 + 15) for a centre, stride 30 for a size: an expectation over 16 bins is at most 15 -- and DEV_S the fp32 statement's
# largest |deviation| / S.  S is the absolute term where x1 + x2 or x2 - x1 cancel and at least |ref64| everywhere, so DEV_S is the relative term too.
# The factor covers what Detect.decode does not reproduce: the kernel's summation order, its own rounding of the centre / size expressions, and
# in the fp16 instance __expf and the reciprocal of the fast sigmoid (common.hpp: v_exp_f32 behind one fp32 multiply by log2(e), v_rcp_f32 at
# 1 ulp) -- a few fp32 steps each; no extra intrinsic term is taken.  Constants: the measurements of `PYTHONPATH=. python tests/detect_ref.py`
# rounded up to two digits; no kernel output enters them.
DEC_DEV = {
    ("box", "f16"): (1.4e-7,), ("cls", "f16"): (8.9e-8, 1.2e-7),
    ("box", "f32"): (1.6e-7,), ("cls", "f32"): (8.9e-8, 1.2e-7),
}
FACTOR = 4.0


def decode_scale(row):
    """S [4, A] of the box rows (see above)."""
    out = []
    for l, (h, w) in enumerate(row["levels"]):
        al = torch.arange(h * w)
        st = STRIDES[l]
        size = torch.full((h * w,), st * 30.0, dtype=torch.float64)
        out.append(torch.stack((st * ((al % w).double() + 15.5), st * ((al // w).double() + 15.5), size, size)))
    return torch.cat(out, 1)


def dec_bound(ref64, fam, dt, row=None):
    if fam == "box":
        return FACTOR * DEC_DEV[(fam, dt)][0] * decode_scale(row).expand_as(ref64)
    a, r = DEC_DEV[(fam, dt)]
    return FACTOR * (a + r * ref64.abs())


def dec_ratio(y, ref64, fam, dt, row=None):
    """(max err / bound, max |err|) of box rows ([B, 4, A], fam "box") or class rows ([B, nc, A], "cls")."""
    err = (y.double() - ref64).abs()
    return float((err / dec_bound(ref64, fam, dt, row)).max()), float(err.max())


def measure_dec_dev():
    """{("box", dtype): (largest |chain32 - ref64| / S,), ("cls", dtype): (largest |chain32 - ref64|, largest relative)} over every decode row."""
    from op_matrix import DECODE_ROWS
    dev = {}
    for row in DECODE_ROWS:
        for dt in row["dtypes"]:
            _, levels, ref = decode_case(row["id"], dt)
            c32 = decode_chain32(row, levels).double()
            err = (c32 - ref).abs()
            dev[("box", dt)] = (max(dev.get(("box", dt), (0.0,))[0], float((err[:, :4] / decode_scale(row)).max())),)
            r = ref[:, 4:]
            rel = torch.where(r > 0, err[:, 4:] / r.clamp(min=1e-300), torch.zeros_like(r))
            a0, r0 = dev.get(("cls", dt), (0.0, 0.0))
            dev[("cls", dt)] = (max(a0, float(err[:, 4:].max())), max(r0, float(rel.max())))
    return dev


def excused_anchors(ref64, dt):
    """[B, A] bool: anchors whose two best reference class scores lie within the class bound of each other -- a correct kernel may name either."""
    cls = ref64[:, 4:]
    if cls.shape[1] < 2:
        return torch.zeros(cls.shape[0], cls.shape[2], dtype=torch.bool)
    top = cls.topk(2, dim=1).values
    return (top[:, 0] - top[:, 1]) <= dec_bound(top[:, 0], "cls", dt)


if __name__ == "__main__":
    for key, dev in sorted(measure_dec_dev().items()):
        print(key, "measured", " ".join("%.4e" % d for d in dev), "  DEC_DEV", DEC_DEV[key])
    print("offset_flips: %d of %d seeded pairs;  fma_flips: %d" % (len(offset_flips()[0]), ROUNDING_SEARCH, len(fma_flips()[0])))
