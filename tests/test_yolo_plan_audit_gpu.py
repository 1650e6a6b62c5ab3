"""The YOLO11 plan audited launch by launch (tests/plan_audit.py): the real Yolo11Plan at the network's own shapes, writing into its own concat
buffers and aliased residuals, every launch against a float64 reference of that one launch on the bytes it actually read, under the per-op
bound of the matrices, and no byte of any plan buffer, packed weight or tail tensor changed outside the launch's output view.

Inputs: `_test_images` of test_yolo_gpu.py; weights: synth.calibrated_yolo_params (activations O(1), 30 - 50 detections); nc = 62.  Per case:
every launch kind the route names was judged, a fused route judged its c3k2_kernel / stem2_kernel / dwpw_kernel tags, and a plain run_eager()
and a captured replay of the same input give pred / det / det_idx / det_count bit-identical to the audited pass (the stepper's
synchronisations hid nothing).  A failure reads `label, kind, kernel tag, err/bound, worst element (b, y, x, c)`.

Measured on the MI355X, one run of this module, RELAX empty (launches judged; worst err/bound per adapter; wall time of the case):
  n_f16          71  stem2 0.195  c3k2 0.200  conv 0.974  dwpw 0.872  dwconv 0.185  attention 0.277  decode 0.327  sppf_pool, nms exact   2.0 s
  n_f16_unfused  89  conv 0.980  dwconv 0.809  attention 0.310  decode 0.225  sppf_pool, nms exact                                        0.2 s
  l_f16         168  conv 0.985  dwconv 0.276  attention 0.298  decode 0.274  sppf_pool, nms exact                                        0.6 s
  n_f32          89  conv 0.118  dwconv 0.425  attention 0.107  decode 0.263  sppf_pool, nms exact                                        0.2 s
  n_f16_160x224  71  stem2 0.182  c3k2 0.200  conv 0.984  dwpw 0.200  dwconv 0.000  attention 0.291  decode 0.230  sppf_pool, nms exact   0.2 s
  n_f16_32x64    71  stem2 0.195  c3k2 0.198  conv 0.963  dwpw 0.200  dwconv 0.000  attention 0.292  decode 0.190  sppf_pool, nms exact   0.2 s
  n_f16_640      71  stem2 0.327  c3k2 0.200  conv 0.986  dwpw 0.315  dwconv 0.188  attention 0.265  decode 0.250  sppf_pool, nms exact   0.2 s
  l_f16_640     168  conv 0.982  dwconv 0.199  attention 0.267  decode 0.250  sppf_pool, nms exact                                        0.8 s
(conv sits next to 1 by construction: u |ref| is half a step of the stored output, which a correct kernel reaches.)  Of n_f16's 2.0 s, 1.4 s
are the first launch's reference: the process's first float64 convolution on the device, paid once by whichever case runs first.
test_yolo11_forward_matches_oracle of the parent commit, same run: n f16 96 x 160 0.24 s, n f32 0.29 s, l f16 96 x 160 0.52 s, n f16 640^2 0.23 s,
l f16 640^2 (batch 2) 1.02 s -- every case is within three times its counterpart but the first-run cost above, and no case needed its
outside-the-view check restricted (OWN_BUFFER_ONLY is empty: l_f16_640 compares every buffer and every packed weight after each launch).
What the 640^2 cases add to the small ones: attn64_kernel<32, 64, 8>, conv_tile_kernel<_Float16, 3, {1, 2}, 16, 128, 2, 2, 8> and
<_Float16, 2, 1, 16, 64, 2, 2, 8> (l), the c3k2 / dwpw / stem2 kernels over many tiles.  No gemm256* kernel is dispatched by the detector at
these shapes (nor by YOLO11-n at batch 32 x 640^2, tried once): the conv matrix remains their only check.
"""
import time

import pytest
import torch

import plan_audit as pa
from circuitvision_amd._lib import F16, F32
from circuitvision_amd.yolo11 import Yolo11Plan, Yolo11Weights
from synth import calibrated_yolo_params
from test_yolo_gpu import _test_images

pytestmark = pytest.mark.gpu
NC = 62


def _case(id, scale, dtype, B, H, W, fuse=True):
    return dict(id=id, scale=scale, dtype=dtype, B=B, H=H, W=W, fuse=fuse)


# the smallest inputs at which each arm exists
CASES = [
    _case("n_f16", "n", F16, 2, 96, 160),                        # fused route; P5 is 3 x 5: attention has N = 15
    _case("n_f16_unfused", "n", F16, 2, 96, 160, fuse=False),    # the chain: bottleneck aliasing, dwconv + 1x1 class branch
    _case("l_f16", "l", F16, 2, 96, 160),                        # c3k blocks, two C2PSA layers, the wide class branch
    _case("n_f32", "n", F32, 2, 96, 160),                        # the f32 instances through the same harness
    _case("n_f16_160x224", "n", F16, 2, 160, 224),               # P5 is 5 x 7: ragged tiles at every level
    _case("n_f16_32x64", "n", F16, 3, 32, 64),                   # degenerate maps (P5 is 1 x 2, P4 is 2 x 4), odd batch
    _case("n_f16_640", "n", F16, 2, 640, 640),                   # the big-shape dispatch
    _case("l_f16_640", "l", F16, 1, 640, 640),                   # the case the whole-model test holds to 0.4 std
]
# cases whose outside-the-view check is restricted to the launch's own output tensors (the time budget of the module's docstring): none
OWN_BUFFER_ONLY = ()

_params = {}


def _weights(case):
    """(input, packed weights) of a case; the calibrated parameters are shared by the cases of one (scale, dtype, shape)."""
    x = _test_images(case["B"], case["H"], case["W"], case["dtype"])
    key = (case["scale"], case["dtype"], case["B"], case["H"], case["W"])
    if key not in _params:
        _params[key] = calibrated_yolo_params(case["scale"], NC, 3, x)
    return x, Yolo11Weights(case["scale"], NC, _params[key], case["dtype"])


def _outputs(yp):
    return {n: getattr(yp, n).clone() for n in ("pred", "det", "det_idx", "det_count")}


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_plan_audit(case):
    t_start = time.time()
    x, wt = _weights(case)
    with pa.recording() as rec:
        yp = Yolo11Plan(wt, case["B"], case["H"], case["W"], torch.cuda.Stream(), fuse_c3k2=case["fuse"])
    yp.set_input_nchw(x)
    torch.cuda.synchronize()
    t_audit = time.time()
    results, failures = pa.audit(yp, rec, case["id"], ledger_all=case["id"] not in OWN_BUFFER_ONLY)
    t_audit = time.time() - t_audit
    audited = _outputs(yp)

    ops = [(label, kind) for label, kind, *_ in yp.plan.ops if kind != "sync"]
    assert [(r["label"], r["kind"]) for r in results] == ops, "the audit skipped a launch"
    named = {kind for _, kind, _ in yp.route.launches()} - {"sync"}
    assert named == {"conv", "stem", "head", "dwconv", "pool", "attention", "decode", "nms"}
    assert {r["kind"] for r in results} == named
    fused = pa.fused_labels(yp.route)
    if case["dtype"] == F16 and case["scale"] == "n":
        assert set(fused.values()) == (set(pa.FUSED_FAMILY) if case["fuse"] else set()), fused
    for label, adapter in fused.items():
        tag = next(r["kernel"] for r in results if r["label"] == label)
        assert tag.split("<")[0] == pa.FUSED_FAMILY[adapter], (label, tag)

    for how in ("run_eager", "run"):                             # a plain eager pass, then a captured replay, of the same input
        getattr(yp.plan, how)()
        torch.cuda.synchronize()
        for name, t in _outputs(yp).items():
            if not torch.equal(t, audited[name]):
                failures.append(f"plan.{how}(): {name} differs from the audited pass")

    worst = " ".join(f"{a} {n}x {w:.3f}" for a, (n, w) in pa.summary(results).items())
    print(f"PLAN-AUDIT {case['id']}: {len(results)} launches judged; worst err/bound per kind: {worst}; detections {yp.det_count.tolist()}; "
          f"audit {t_audit:.1f} s, case {time.time() - t_start:.1f} s")
    print(f"PLAN-AUDIT {case['id']} kernels: {sorted({r['kernel'] for r in results})}")
    slow = sorted(results, key=lambda r: -r["seconds"])[:3]
    print(f"PLAN-AUDIT {case['id']} slowest: " + "; ".join(f"{r['label']} {r['seconds']:.2f} s" for r in slow))
    assert not failures, f"{case['id']}:\n  " + "\n  ".join(failures)


def _after(yp, rec, label, what):
    """Replaces launch `label` of the plan by itself followed by what(output View) (plain tensor writes, then a synchronisation)."""
    k = next(i for i, op in enumerate(yp.plan.ops) if op[0] == label)
    lab, kind, thunk, b, f = yp.plan.ops[k]
    dst = yp.plan.keep[rec.keep_len[k] - 1][3]

    def wrapped(sp=None):
        thunk(sp)
        torch.cuda.synchronize()
        what(dst)
        torch.cuda.synchronize()

    yp.plan.ops[k] = (lab, kind, wrapped, b, f)
    return dst


def test_the_audit_sees_planted_damage_in_the_real_plan():
    """The stepper on the GPU, on YOLO11-n at 96 x 160: one launch followed by a write to the live channel right in front of its output slice
    (model.6.m.0.cv3 writes channels [2c, 3c) of model.6's concat buffer; [0, 2c) hold cv1's output), another followed by 2^-4 added to one
    element of its own output.  The audit reports exactly these two, each where it happened: the launches downstream of the wrong element read
    it as their input and are judged on it, so nothing else fails."""
    case = CASES[0]
    x, wt = _weights(case)
    with pa.recording() as rec:
        yp = Yolo11Plan(wt, case["B"], case["H"], case["W"], torch.cuda.Stream())
    yp.set_input_nchw(x)
    torch.cuda.synchronize()

    def neighbour(dst):
        assert dst.c0 > 0
        dst.buf.t[1, 2, 3, dst.c0 - 1] += 1.0

    def own(dst):
        dst.tensor()[1, 4, 7, 5] += 0.0625

    _after(yp, rec, "model.6.m.0.cv3", neighbour)
    _after(yp, rec, "model.13.cv2", own)
    results, failures = pa.audit(yp, rec, case["id"])
    print("\n".join(failures))
    assert len(failures) == 2, failures
    assert failures[0].startswith("model.6.m.0.cv3, conv,") and "outside the output view" in failures[0] and "(1, 2, 3, " in failures[0]
    assert failures[1].startswith("model.13.cv2, conv,") and "err/bound" in failures[1] and "worst element (1, 4, 7, 5)" in failures[1]
