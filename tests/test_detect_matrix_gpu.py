"""The detector-tail matrix (tests/op_matrix.py NMS_ROWS, DECODE_ROWS): yolo_nms_kernel at every edge of its data-dependent branches -- keys in LDS or
in the workspace, four or sixteen waves, geometry in LDS or not, n = 0 .. A = P, max_det 1 .. NMS_MAX_DET, the thresholds' edges, degenerate
boxes, pairs whose verdict hangs on fp32 rounding, ultralytics' max_nms -- and detect_decode_kernel at its seams, each pinned by the tag
cvmi_last_kernel() reports.  NMS is compared exactly (count, anchor indices, six columns) with oracle/nms.py on inputs that hold exactly the
stated number of candidates; the decode with its fp64 statement under the bound of tests/detect_ref.py, measured on the CPU, never from a kernel.
tests/test_detect_ref_cpu.py proves on the CPU that these comparisons catch the classic mistakes.

Every case asserts the tag first, then the values, then that rows behind the count, guard elements around every output and the bytes around the
workspace are untouched.  Inputs hold NaN in every channel the decode must not use."""
import ctypes as C
import time

import pytest
import torch

from circuitvision_amd import _lib
from circuitvision_amd._lib import F16, F32
from oracle import nms as onms
import detect_ref as R
from op_matrix import DECODE_REFUSED, DECODE_ROWS, NMS_REFUSED, NMS_ROWS, decode_tag, nms_tag, nms_workspace

pytestmark = pytest.mark.gpu
CODE = {"f16": F16, "f32": F32}
VEC = {"f16": 8, "f32": 4}
GUARD = 64                                              # sentinel elements on both sides of every output
SENT_I = -12288


class Guarded:
    """A device tensor of `shape` with GUARD sentinel elements before and after it."""

    def __init__(self, shape, dtype):
        self.fill = R.SENTINEL if dtype.is_floating_point else (0xA5 if dtype == torch.uint8 else SENT_I)
        n = 1
        for s in shape:
            n *= s
        self.whole = torch.full((n + 2 * GUARD,), self.fill, dtype=dtype, device="cuda")
        self.t = self.whole[GUARD:GUARD + n].view(shape)
        self.n = n

    def ptr(self):
        return self.t.data_ptr()

    def guards_intact(self):
        w = self.whole.cpu()
        return bool((w[:GUARD] == self.fill).all()) and bool((w[GUARD + self.n:] == self.fill).all())


# ---- cvmi_yolo_nms_best / cvmi_yolo_nms -----------------------------------------------------------------------------------------------------------
def _launch_nms(lib, row, pred_d, best, entry):
    """(tag, det, idx, cnt on the CPU, failures of the memory checks) of one launch through `entry` ("best" | "nms")."""
    B, nc, A, md = row["B"], row["nc"], row["A"], row["max_det"]
    det, idx, cnt = Guarded((B, md, 6), torch.float32), Guarded((B, md), torch.int32), Guarded((B,), torch.int32)
    nbytes = lib.cvmi_yolo_nms_workspace(B, A)
    assert nbytes == nms_workspace(B, A), (nbytes, nms_workspace(B, A))
    ws = Guarded((nbytes,), torch.uint8)
    lib.cvmi_last_kernel()
    torch.cuda.synchronize()
    if entry == "best":
        rc = lib.cvmi_yolo_nms_best(pred_d.data_ptr(), best[0].data_ptr(), best[1].data_ptr(), B, nc, A, row["conf"], row["iou"], md, row["max_wh"],
                                    det.ptr(), idx.ptr(), cnt.ptr(), ws.ptr(), None)
    else:
        rc = lib.cvmi_yolo_nms(pred_d.data_ptr(), B, nc, A, row["conf"], row["iou"], md, row["max_wh"], det.ptr(), idx.ptr(), cnt.ptr(), ws.ptr(), None)
    _lib.check(rc, "yolo_nms " + entry)
    torch.cuda.synchronize()
    tag = lib.cvmi_last_kernel().decode()
    bad = [name for name, g in (("det", det), ("idx", idx), ("count", cnt), ("workspace", ws)) if not g.guards_intact()]
    return tag, det.t.cpu(), idx.t.cpu(), cnt.t.cpu(), ["guard elements around %s were written" % n for n in bad]


def _compare_nms(row, det, idx, cnt, ref, ref_idx):
    failures = []
    for b in range(row["B"]):
        n, want = int(cnt[b]), ref[b].shape[0]
        if n != want:
            failures.append(f"image {b}: {n} detections, reference {want}")
            continue
        if not torch.equal(idx[b, :n].long(), ref_idx[b]):
            failures.append(f"image {b}: anchor indices differ")
        if not torch.equal(det[b, :n], ref[b]):
            failures.append(f"image {b}: detections differ, max |diff| {float((det[b, :n] - ref[b]).abs().max()):.3e}")
        if not (bool((det[b, n:] == R.SENTINEL).all()) and bool((idx[b, n:] == SENT_I).all())):
            failures.append(f"image {b}: rows behind the count were written")
    return failures


@pytest.mark.parametrize("rid", [r["id"] for r in NMS_ROWS])
def test_nms_matrix(rid):
    lib = _lib.load()
    t0 = time.time()
    row, pred, ref, ref_idx = R.nms_case(rid)
    t_ref = time.time() - t0
    pred_d = pred.cuda()
    best = tuple(t.cuda() for t in R.best_of(pred))
    tag, det, idx, cnt, failures = _launch_nms(lib, row, pred_d, best, "best")
    print(f"NMS-MATRIX {rid}: {tag or '(untagged)'}  gk {row['gk']} nthr {row['nthr']} geo_lds {row['geo_lds']} Ps {row['Ps']} of P {row['P']}  "
          f"counts {cnt.tolist()[:4]} reference {[d.shape[0] for d in ref][:4]}  ref {t_ref:.2f} s, all {time.time() - t0:.2f} s")
    assert tag == row["expect"] == nms_tag(row["gk"]), f"{rid}: kernel {tag!r}, expected {row['expect']!r}"
    failures += _compare_nms(row, det, idx, cnt, ref, ref_idx)
    if row["entry"] == "both":
        tag2, det2, idx2, cnt2, f2 = _launch_nms(lib, row, pred_d, best, "nms")
        assert tag2 == row["expect"], f"{rid}: cvmi_yolo_nms ran {tag2!r}, expected {row['expect']!r}"
        failures += ["cvmi_yolo_nms: " + f for f in f2]
        if not (torch.equal(cnt, cnt2) and torch.equal(idx, idx2) and torch.equal(det, det2)):
            failures.append("cvmi_yolo_nms and cvmi_yolo_nms_best differ")
    assert not failures, f"{rid}:\n  " + "\n  ".join(failures)


# ---- cvmi_detect_decode ------------------------------------------------------------------------------------------------------------------------------
def _decode_buffers(row, dt, levels):
    """Device inputs of a decode row: per level a [B, h, w, ld] buffer of NaN holding the 64 box / nc class channels at its front."""
    td, v = R.TDT[dt], VEC[dt]
    ncp = (row["nc"] + v - 1) // v * v
    box_ld, cls_ld = 64 + row["box_extra"], ncp + row["cls_extra"]
    boxes, clss = [], []
    for box, cls in levels:
        B, h, w, _ = box.shape
        bb = torch.full((B, h, w, box_ld), float("nan"), dtype=td)
        bb[..., :64] = box.to(td)
        cb = torch.full((B, h, w, cls_ld), float("nan"), dtype=td)
        cb[..., :row["nc"]] = cls.to(td)
        boxes.append(bb.cuda())
        clss.append(cb.cuda())
    return boxes, clss, box_ld, cls_ld


def _decode_call(lib, row, dt, boxes, clss, box_ld, cls_ld, pred, bs, bc, write_cls, nc=None):
    nl = len(boxes)
    args = ((C.c_void_p * nl)(*[t.data_ptr() for t in boxes]), (C.c_int * nl)(*[box_ld] * nl), (C.c_void_p * nl)(*[t.data_ptr() for t in clss]),
            (C.c_int * nl)(*[cls_ld] * nl), (C.c_int * nl)(*[t.shape[1] for t in boxes]), (C.c_int * nl)(*[t.shape[2] for t in boxes]),
            (C.c_float * nl)(*R.STRIDES[:nl]))
    return lib.cvmi_detect_decode(*args, nl, row["B"], row["nc"] if nc is None else nc, CODE[dt], pred, bs, bc, write_cls, None)


DECODE_CASES = [(r["id"], dt) for r in DECODE_ROWS for dt in r["dtypes"]]


@pytest.mark.parametrize("rid,dt", DECODE_CASES, ids=["%s-%s" % c for c in DECODE_CASES])
def test_decode_matrix(rid, dt):
    lib = _lib.load()
    row, levels, ref = R.decode_case(rid, dt)
    B, nc, A = row["B"], row["nc"], row["A"]
    boxes, clss, box_ld, cls_ld = _decode_buffers(row, dt, levels)
    pred, bs, bc = Guarded((B, 4 + nc, A), torch.float32), Guarded((B * A,), torch.float32), Guarded((B * A,), torch.int32)
    lib.cvmi_last_kernel()
    torch.cuda.synchronize()
    _lib.check(_decode_call(lib, row, dt, boxes, clss, box_ld, cls_ld, pred.ptr(), bs.ptr(), bc.ptr(), 1), "detect_decode")
    torch.cuda.synchronize()
    tag = lib.cvmi_last_kernel().decode()
    assert tag == decode_tag(dt), f"{rid} {dt}: kernel {tag!r}, expected {decode_tag(dt)!r}"
    got, score, cls = pred.t.cpu(), bs.t.cpu().view(B, A), bc.t.cpu().view(B, A).long()
    failures = []
    if not bool(torch.isfinite(got).all()):
        failures.append("non-finite output: a NaN channel was used")
    rb, eb = R.dec_ratio(got[:, :4], ref[:, :4], "box", dt, row)
    rc, ec = R.dec_ratio(got[:, 4:], ref[:, 4:], "cls", dt)
    print(f"DECODE-MATRIX {rid} {dt}: {tag}  box max|err| {eb:.3e} err/bound {rb:.3f}   cls max|err| {ec:.3e} err/bound {rc:.3f}")
    if not rb <= 1.0:
        failures.append(f"box rows: err/bound {rb:.3f}")
    if not rc <= 1.0:
        failures.append(f"class rows: err/bound {rc:.3f}")
    own_s, own_c = R.best_ref(got[:, 4:])
    if not (torch.equal(score, own_s) and torch.equal(cls, own_c)):
        failures.append("best score / class are not the first maximum of the kernel's own class rows")
    if row["kind"] == "rand":
        wrong = (cls != R.best_ref(ref[:, 4:])[1]) & ~R.excused_anchors(ref, dt)
        if bool(wrong.any()):
            failures.append(f"best class differs from the reference's on {int(wrong.sum())} anchors whose top-two gap exceeds the bound")
    elif not torch.equal(cls, R.decode_exact_cls(row, levels)):
        failures.append("best class is not the first maximum of the logits")
    failures += ["guard elements around %s were written" % n for n, g in (("pred", pred), ("best_score", bs), ("best_cls", bc)) if not g.guards_intact()]
    if row["optional"]:
        p2 = Guarded((B, 4 + nc, A), torch.float32)
        lib.cvmi_last_kernel()
        _lib.check(_decode_call(lib, row, dt, boxes, clss, box_ld, cls_ld, p2.ptr(), None, None, 0), "detect_decode, boxes only")
        torch.cuda.synchronize()
        assert lib.cvmi_last_kernel().decode() == decode_tag(dt)
        g2 = p2.t.cpu()
        if not (torch.equal(g2[:, :4], got[:, :4]) and bool((g2[:, 4:] == R.SENTINEL).all()) and p2.guards_intact()):
            failures.append("write_cls = 0: box rows differ or class rows were written")
        p3 = Guarded((B, 4 + nc, A), torch.float32)
        _lib.check(_decode_call(lib, row, dt, boxes, clss, box_ld, cls_ld, p3.ptr(), None, None, 1), "detect_decode, no best class")
        torch.cuda.synchronize()
        if not (torch.equal(p3.t.cpu(), got) and p3.guards_intact()):
            failures.append("without best-class outputs pred differs")
    if row["chain"]:                                                      # the kernel's own best arrays feed cvmi_yolo_nms_best
        nrow = dict(B=B, nc=nc, A=A, max_det=300, conf=0.25, iou=0.7, max_wh=7680.0)
        ntag, det, idx, cnt, f2 = _launch_nms(lib, nrow, pred.t, (bs.t, bc.t), "best")
        assert ntag == nms_tag(False), ntag
        want, want_idx = onms.yolo_nms(got, 0.25, 0.7, 300, return_indices=True)
        assert min(d.shape[0] for d in want) >= 10, "the chain row must keep something"
        failures += f2 + _compare_nms(nrow, det, idx, cnt, want, want_idx)
    assert not failures, f"{rid} {dt}:\n  " + "\n  ".join(failures)


# ---- argument rejection: every call below returns before any launch ---------------------------------------------------------------------------------
def _rejected(lib, rc, text):
    assert rc != 0
    err = lib.cvmi_last_error().decode()
    assert text in err, err
    assert lib.cvmi_last_kernel().decode() == "", "a rejected call must not reach a launch"


@pytest.mark.parametrize("case", NMS_REFUSED, ids=[c["id"] for c in NMS_REFUSED])
def test_nms_rejects_what_it_cannot_hold(case):
    lib = _lib.load()
    B, nc, A = case["B"], case["nc"], case["A"]
    md = case["max_det"]
    pred = torch.zeros(B, 4 + nc, A, device="cuda")
    bs, bc = torch.zeros(B, A, device="cuda"), torch.zeros(B, A, dtype=torch.int32, device="cuda")
    det, idx, cnt = torch.zeros(B, md, 6, device="cuda"), torch.zeros(B, md, dtype=torch.int32, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda")
    ws = torch.zeros(B * A * 28 + 256 + 16 + B * 8 * 131072, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    lib.cvmi_last_kernel()
    _rejected(lib, lib.cvmi_yolo_nms_best(pred.data_ptr(), bs.data_ptr(), bc.data_ptr(), B, nc, A, 0.25, 0.7, md, 7680.0, det.data_ptr(), idx.data_ptr(),
                                          cnt.data_ptr(), ws.data_ptr(), None), case["text"])
    _rejected(lib, lib.cvmi_yolo_nms(pred.data_ptr(), B, nc, A, 0.25, 0.7, md, 7680.0, det.data_ptr(), idx.data_ptr(), cnt.data_ptr(), ws.data_ptr(), None),
              case["text"])
    torch.cuda.synchronize()
    assert float(det.abs().max()) == 0.0 and int(cnt.abs().max()) == 0


@pytest.mark.parametrize("case", DECODE_REFUSED, ids=[c["id"] for c in DECODE_REFUSED])
def test_decode_rejects_what_it_cannot_hold(case):
    lib = _lib.load()
    dt, nc = case["dt"], case["nc"]
    row = dict(B=1, nc=nc, box_extra=0, cls_extra=0)
    levels = [(torch.zeros(1, 2, 2, 64), torch.zeros(1, 2, 2, nc))]
    boxes, clss, box_ld, cls_ld = _decode_buffers(row, dt, levels)
    pred = torch.zeros(1, 4 + nc, 4, device="cuda")
    bs, bc = torch.zeros(4, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    lib.cvmi_last_kernel()
    best = case.get("best")
    _rejected(lib, _decode_call(lib, row, dt, boxes, clss, box_ld, cls_ld, pred.data_ptr(), None if best == "cls" else bs.data_ptr(),
                                None if best == "score" else bc.data_ptr(), 1), case["text"])
    torch.cuda.synchronize()
    assert float(pred.abs().max()) == 0.0
