"""In-situ audit of a Yolo11Plan: every launch of the real plan, run alone, against a float64 reference of that ONE launch computed from the
bytes the launch actually read, under the per-op bound the matrices already derived (tests/test_conv_matrix_gpu.py, test_attention_matrix_gpu.py,
fused_ref.py, helper_ref.py, detect_ref.py), plus the in-situ form of their sentinel check: no byte of any plan buffer outside the launch's
output view may change.  An error is judged where it is made, so the ~750-fold growth from input to head that forces the whole-model tests to
0.2 - 0.4 of a standard deviation never enters.  Importing this module needs neither a GPU nor the library; tests/test_plan_audit_cpu.py runs
every judge on the CPU against chain32 and against named mutants.

Pairing.  Every op_* wrapper of engine.py appends its operands to plan.keep just before it calls plan.add, so `recording()` wraps Plan.add and
notes len(plan.keep) per op (and wraps Buf.__init__ to collect the plan's buffers).  What a keep entry does not carry (the activation of
op_dwconv, the channel count of op_sppf_pool) is read from the launch's own argument tuple in the thunk's closure; decode and NMS take their
operands from the Yolo11Plan attributes.  `resolve(label, kind, route)` names the adapter of a launch from the route alone (no GPU): `sync`
entries (fork / join) are the only ones without one, anything else unknown raises.

Weights are taken as stored: PackedConv.w[:N, :K] as [N, KH, KW, Cin] in the plan's dtype with the f32 bias, PackedDW.w as [9][C].

Bounds (no new constants; every figure is the matrix's own, RELAX stays empty unless chain32 on the same inputs shows a correct
fp32-accumulating implementation exceeds the bound too):
  conv       |y - ref| <= u |ref| + L (K + 2) 2^-24 A + e_act + 1e-7  (+ L2 u |t| where the epilogue rounds twice: a 16-bit output with a residual)
             with t = TO(act(acc + bias)), y = TO(act2(t + res)) as csrc/conv_epilogue.hpp states it; two sources, `up` and out_hw stated here
  attention  3 u sum_k p_k |v_k| + u |ref| + 1e-6  (f32: 1e-5 + 1e-4 |ref|)
  sppf_pool  exact;  nms: exact against the oracle NMS of the GPU's own pred
  c3k2, stem2, dwpw, dwconv3x3, decode: the module's own FACTOR (4) and RTOL, with the absolute term measured per launch on that launch's
             inputs: FACTOR x max |ref(float32) - ref(float64)|.  dwconv3x3 with a 16-bit output adds the same measurement with an f32 output,
             as helper_ref.ATOL does (an output next to 0 has fp16 steps far below the fp32 arithmetic's error).  Decode keeps detect_ref's
             forms: box rows FACTOR DEV_S S, class rows FACTOR (DEV_ABS + DEV_REL |ref|), the three deviations measured on the launch's inputs.
The kernel under test never enters a bound."""
import contextlib
import time

import torch
import torch.nn.functional as F

import detect_ref
import fused_ref
import helper_ref
from circuitvision_amd._lib import ACT_GELU, ACT_NONE, ACT_RELU, ACT_SILU, F16, F32, AttnDesc, C3k2Desc, ConvDesc, DwPwDesc

KINDS = ("conv", "c3k2", "stem2", "dwpw", "dwconv", "sppf_pool", "attention", "decode", "nms")
FUSED_FAMILY = {"c3k2": "c3k2_kernel", "stem2": "stem2_kernel", "dwpw": "dwpw_kernel"}
CONV_FAMILIES = ("conv_tile_kernel", "igemm_kernel", "gemm256_kernel", "gemm256p_kernel", "gemm256x192_kernel", "gemm256x192r_kernel")
UNIT = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8, torch.float32: 2.0 ** -24}
ACT_REF = {ACT_NONE: lambda v: v, ACT_RELU: torch.relu, ACT_SILU: F.silu, ACT_GELU: F.gelu}
SLOPE = {ACT_NONE: 1.0, ACT_RELU: 1.0, ACT_SILU: 1.10, ACT_GELU: 1.13}
STORED = {torch.float16: "f16", torch.float32: "f32"}
# per-launch relaxations (case id, label) -> factor, each with its measured ratio and the chain32 evidence beside it: none needed
RELAX = {}


# ---- which adapter a launch takes (no GPU) ------------------------------------------------------------------------------------------------------
def fused_labels(route):
    """{label: adapter} of the launches the route calls fused."""
    out = {"model.0-1": "stem2"} if route.stem == "fused" else {}
    for name, mode in route.c3k2.items():
        if mode != "chain":
            out[name if mode == "fused_cv1" else f"{name}.fused"] = "c3k2"
    det = route.layers[-1].name
    for i, mode in enumerate(route.cls):
        if mode == "dwpw":
            out.update({f"{det}.cv3.{i}.0": "dwpw", f"{det}.cv3.{i}.1-2": "dwpw"})
    return out


def resolve(label, kind, route):
    """Adapter name of a launch, None for a `sync` entry; an unknown kind raises."""
    if kind == "sync":
        return None
    fused = fused_labels(route)
    if label in fused:
        assert kind in ("conv", "stem", "head"), (label, kind)
        return fused[label]
    table = {"conv": "conv", "stem": "conv", "head": "conv", "dwconv": "dwconv", "pool": "sppf_pool", "attention": "attention",
             "decode": "decode", "nms": "nms"}
    if kind not in table:
        raise KeyError(f"{label}: launch kind {kind!r} has no audit adapter")
    return table[kind]


def kernel_fits(adapter, kernel):
    """The recorded kernel tag belongs to the adapter's family ("" / None: a dispatcher that does not tag itself, or a case that was not run)."""
    if not kernel:
        return True
    family = kernel.split("<")[0]
    if adapter in FUSED_FAMILY:
        return family == FUSED_FAMILY[adapter]
    return {"conv": family in CONV_FAMILIES, "sppf_pool": family.startswith("sppf_pool"), "attention": family.startswith("attn"),
            "decode": family == "detect_decode_kernel", "nms": family == "yolo_nms_kernel", "dwconv": family.startswith("dwconv")}[adapter]


# ---- small helpers ------------------------------------------------------------------------------------------------------------------------------
def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


@contextlib.contextmanager
def _plain():
    """References run on plain im2col + BLAS statements in the dtype they name, on either device: no convolution library picks an algorithm."""
    was = torch.backends.cudnn.enabled
    torch.backends.cudnn.enabled = False
    try:
        yield
    finally:
        torch.backends.cudnn.enabled = was


def worst(err, bound):
    """(largest err / bound, its index tuple) over tensors of one shape."""
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)           # (an exact element passes a zero bound)
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    i = int(torch.argmax(r))
    return float(r.flatten()[i]), tuple(int(v) for v in torch.unravel_index(torch.tensor(i), r.shape))


def _exact(got, ref):
    bad = got != ref
    n = int(bad.sum())
    if not n:
        return 0.0, (), ""
    i = tuple(int(v) for v in torch.unravel_index(torch.nonzero(bad.flatten())[0, 0].cpu(), bad.shape))
    return float("inf"), i, f"{n} of {bad.numel()} elements differ; first: got {float(got[i])} ref {float(ref[i])}"


# ---- conv ---------------------------------------------------------------------------------------------------------------------------------------
CONV_MUTANTS = ("act_after_res", "tap_wraps_row")


def conv_input(srcs, ups):
    """The NHWC sources (a source with up = 1 at half resolution: nearest 2x) as one logical [B, H, W, c0 + c1] input."""
    full = [t.repeat_interleave(2, 1).repeat_interleave(2, 2) if up else t for t, up in zip(srcs, ups)]
    assert all(up in (0, 1) for up in ups)
    return full[0] if len(full) == 1 else torch.cat(full, -1)


def conv_sum(X, w, p, dtype, mutant=None):
    """sum_k A[m, k] w[n, k] as [B, OH, OW, N] in `dtype`: X NHWC, w [N, KH, KW, Cin], p = dict(stride, pad, OH, OW).  Zero padding of `pad` on
    every side, the natural output cropped to OH x OW (out_hw).  mutant tap_wraps_row: the tap one column past the image reads the NHWC
    neighbour in memory, pixel 0 of the next row."""
    B, H, W, ct = X.shape
    N, KH, KW, cin = w.shape
    assert cin == ct, (cin, ct)
    s, pad, OH, OW = p["stride"], p["pad"], p["OH"], p["OW"]
    if KH == 1 and KW == 1 and s == 1 and pad == 0:
        assert mutant is None
        return (X.reshape(-1, ct).to(dtype) @ w.reshape(N, ct).to(dtype).t()).view(B, H, W, N)[:, :OH, :OW]
    x = nchw(X).to(dtype)
    xp = F.pad(x, (pad, pad, pad, pad))
    if mutant == "tap_wraps_row":
        assert pad >= 1 and H > 1
        xp[:, :, pad:pad + H - 1, W + pad] = x[:, :, 1:, 0]
    wm = w.permute(0, 3, 1, 2).reshape(N, -1).to(dtype).t()              # rows in (c, ky, kx) order, as F.unfold lists them
    OHf, OWf = (H + 2 * pad - KH) // s + 1, (W + 2 * pad - KW) // s + 1
    assert OH <= OHf and OW <= OWf
    out = []
    for b in range(B):                                                    # per image: bounds the size of the unfolded matrix
        cols = F.unfold(xp[b:b + 1], (KH, KW), stride=s)[0]
        out.append((cols.t() @ wm).view(OHf, OWf, N)[:OH, :OW])
    return torch.stack(out)


def conv_stored(i, p, dtype=torch.float32, mutant=None):
    """The launch as an implementation that accumulates in `dtype` stores it: both lines of the epilogue contract with their roundings."""
    to = p["out"]
    aar = bool(p["act_after_res"]) != (mutant == "act_after_res")
    act = ACT_REF[p["act"]]
    X = conv_input(i["srcs"], p["ups"])
    v = conv_sum(X, i["w"], p, dtype, mutant if mutant == "tap_wraps_row" else None) + i["bias"].to(dtype)
    t = (v if aar else act(v)).to(to)
    if i.get("res") is None and not aar:
        return t
    r = i["res"].to(dtype) if i.get("res") is not None else 0.0
    y = t.to(dtype) + r
    return (act(y) if aar else y).to(to)


def judge_conv(i, p, got):
    """i: srcs [NHWC tensors], w [N, KH, KW, Cin], bias f32 [N], res NHWC or None.  p: stride, pad, OH, OW, ups, act, act_after_res, out (the
    output's torch dtype), fast (16-bit mode: the fast activations).  Bound: the module's docstring."""
    d = torch.float64
    to, act, aar = p["out"], p["act"], bool(p["act_after_res"])
    u, L = UNIT[to], SLOPE[act]
    X = conv_input(i["srcs"], p["ups"])
    K = i["w"].shape[1] * i["w"].shape[2] * i["w"].shape[3]
    bd = i["bias"].to(d)
    v = conv_sum(X, i["w"], p, d) + bd
    A = conv_sum(X.abs(), i["w"].abs(), p, d) + bd.abs()
    t = v if aar else ACT_REF[act](v)
    ref = t
    has_res = i.get("res") is not None
    if has_res or aar:
        ref = t + (i["res"].to(d) if has_res else 0.0)
        if aar:
            ref = ACT_REF[act](ref)
    e_act = 0.0
    if p["fast"] and act == ACT_GELU:
        e_act = 2.5e-5
    elif p["fast"] and act == ACT_SILU:
        e_act = 4 * 2.0 ** -24 * (ref if aar else t).abs()
    bound = u * ref.abs() + L * (K + 2) * 2.0 ** -24 * A + e_act + 1e-7
    if to != torch.float32 and (has_res or aar):
        bound = bound + (L if aar else 1.0) * u * t.abs()
    ratio, idx = worst((got.to(d) - ref).abs(), bound)
    return ratio, idx, f"got {float(got[idx]):.6e} ref {float(ref[idx]):.6e} bound {float(bound[idx]):.3e}"


# ---- the fused kernels and the helpers: FACTOR x chain32's own deviation on these inputs ----------------------------------------------------------
def _tol(got, ref64, ref32, rtol, factor, extra_atol=0.0):
    """got, ref64, ref32 in one layout.  |got - ref64| <= factor max|ref32 - ref64| + extra + rtol |ref64|."""
    ref64 = ref64.double()
    atol = factor * float((ref32.double() - ref64).abs().max()) + extra_atol
    bound = atol + rtol * ref64.abs()
    ratio, idx = worst((got.double() - ref64).abs(), bound)
    return ratio, idx, f"got {float(got[idx]):.6e} ref {float(ref64[idx]):.6e} atol {atol:.3e}"


def c3k2_out(i, p, dtype, mutant=None):
    with _plain():
        return nhwc(fused_ref.c3k2_ref(nchw(i["x"]), i["w0"], i["b0"], i["w1"], i["b1"], i["w2"], i["b2"], i["w3"], i["b3"], p["shortcut"], p["fuse_cv1"],
                                       dtype, mutant))


def judge_c3k2(i, p, got):
    return _tol(got, c3k2_out(i, p, torch.float64), c3k2_out(i, p, torch.float32), fused_ref.RTOL, fused_ref.FACTOR)


def s2d_to_image(x):
    """Space-to-depth(2) NHWC [B, H2, W2, 16] (12 real channels, (sy, sx, rgb) order) -> image NCHW [B, 3, 2 H2, 2 W2] (Yolo11Plan.input_nchw)."""
    B, H2, W2, _ = x.shape
    return x[..., :12].reshape(B, H2, W2, 2, 2, 3).permute(0, 5, 1, 3, 2, 4).reshape(B, 3, H2 * 2, W2 * 2)


def stem_weight_3x3(w2):
    """Yolo11Weights._stem inverted: the stored 2x2 / 16-channel weight NCHW [N, 16, 2, 2] -> the 3x3 / 3-channel weight it restates.  Every
    stored entry the 3x3 form has no tap for must be zero (asserted), so the two are the same function of the image."""
    N = w2.shape[0]
    w = torch.zeros(N, 3, 3, 3, dtype=w2.dtype, device=w2.device)
    used = torch.zeros_like(w2, dtype=torch.bool)
    m = {0: (0, 1), 1: (1, 0), 2: (1, 1)}
    for ky in range(3):
        for kx in range(3):
            (ty, sy), (tx, sx) = m[ky], m[kx]
            c = (sy * 2 + sx) * 3
            w[:, :, ky, kx] = w2[:, c:c + 3, ty, tx]
            used[:, c:c + 3, ty, tx] = True
    assert not bool(w2[~used].any()), "the stored stem weight has entries outside the 3x3 window"
    return w


def stem2_out(i, p, dtype, mutant=None):
    with _plain():
        return nhwc(fused_ref.stem2_ref(s2d_to_image(i["x"]), stem_weight_3x3(i["w0"]), i["b0"], i["w1"], i["b1"], dtype, mutant))


def judge_stem2(i, p, got):
    return _tol(got, stem2_out(i, p, torch.float64), stem2_out(i, p, torch.float32), fused_ref.RTOL, fused_ref.FACTOR)


def dwpw_out(i, p, dtype, mutant=None):
    with _plain():
        return nhwc(fused_ref.dwpw_ref(nchw(i["x"]), i["wd"], i["bd"], i["w1"], i["b1"], i.get("w2"), i.get("b2"), dtype, mutant))


def judge_dwpw(i, p, got):
    return _tol(got, dwpw_out(i, p, torch.float64), dwpw_out(i, p, torch.float32), fused_ref.RTOL, fused_ref.FACTOR)


def dwconv_out(i, p, dtype, mutant=None, stored=None):
    res = nchw(i["res"]) if i.get("res") is not None else None
    return nhwc(helper_ref.dwconv_ref(nchw(i["x"]), i["w"], i["b"], res, p["act"], stored or p["stored"], dtype, mutant))


def judge_dwconv(i, p, got):
    """p: act ("none" | "silu"), stored ("f16" | "f32")."""
    extra = 0.0
    if p["stored"] != "f32":                               # helper_ref: ATOL["dwconv3x3_f16"] += ATOL["dwconv3x3_f32"]
        extra = helper_ref.FACTOR * float((dwconv_out(i, p, torch.float32, stored="f32").double() - dwconv_out(i, p, torch.float64, stored="f32")).abs().max())
    return _tol(got, dwconv_out(i, p, torch.float64), dwconv_out(i, p, torch.float32), helper_ref.RTOL[p["stored"]], helper_ref.FACTOR, extra)


def sppf_out(i, p, mutant=None):
    c = i["x"].shape[-1]
    return nhwc(helper_ref.sppf_ref(nchw(i["x"]).float(), mutant)[:, c:]).to(i["x"].dtype)


def judge_sppf_pool(i, p, got):
    return _exact(got, sppf_out(i, p))


# ---- attention ----------------------------------------------------------------------------------------------------------------------------------
def attention_out(i, p, dtype=torch.float64):
    """i: q, k [B, heads, N, dqk], v [B, heads, N, dv] -> (softmax(q k^T scale) v, softmax(q k^T scale) |v|) in `dtype`."""
    pr = torch.softmax((i["q"].to(dtype) @ i["k"].to(dtype).transpose(-1, -2)) * p["scale"], -1)
    return pr @ i["v"].to(dtype), pr @ i["v"].to(dtype).abs()


def judge_attention(i, p, got):
    """got [B, heads, Nq, dv].  Bound: tests/test_attention_matrix_gpu.py."""
    ref, absref = attention_out(i, p)
    if p["out"] == torch.float32:
        bound = 1e-5 + 1e-4 * ref.abs()
    else:
        u = UNIT[p["out"]]
        bound = 3 * u * absref + u * ref.abs() + 1e-6
    ratio, idx = worst((got.double() - ref).abs(), bound)
    return ratio, idx, f"[b, head, token, d]: got {float(got[idx]):.6e} ref {float(ref[idx]):.6e} bound {float(bound[idx]):.3e}"


# ---- decode and NMS (CPU) -----------------------------------------------------------------------------------------------------------------------
def decode_bounds(levels, nc):
    """(ref64 [B, 4 + nc, A], bound of the same shape) from the launch's inputs alone: detect_ref's forms with the fp32 statement's deviations
    (oracle.yolo11.Detect.decode) measured on these inputs."""
    row = dict(nc=nc, levels=[tuple(b.shape[1:3]) for b, _ in levels])
    ref = detect_ref.decode_ref(levels)
    err = (detect_ref.decode_chain32(row, levels).double() - ref).abs()
    S = detect_ref.decode_scale(row)
    dev_s = float((err[:, :4] / S).max())
    r = ref[:, 4:]
    dev_abs = float(err[:, 4:].max())
    dev_rel = float(torch.where(r > 0, err[:, 4:] / r.clamp(min=1e-300), torch.zeros_like(r)).max())
    bound = torch.cat((detect_ref.FACTOR * dev_s * S.expand_as(ref[:, :4]), detect_ref.FACTOR * (dev_abs + dev_rel * r.abs())), 1)
    return ref, bound


def judge_decode(i, p, got):
    """i: levels [(box [B, h, w, 64], cls [B, h, w, nc]) f32 CPU]; got: dict(pred, best_score, best_cls) CPU.  The best arrays must be the first
    maximum of the kernel's own class rows (exact), as the decode matrix holds them."""
    ref, bound = decode_bounds(i["levels"], p["nc"])
    pred = got["pred"]
    ratio, idx = worst((pred.double() - ref).abs(), bound)
    note = f"[b, row, anchor]: got {float(pred[idx]):.6e} ref {float(ref[idx]):.6e} bound {float(bound[idx]):.3e}"
    s, c = detect_ref.best_ref(pred[:, 4:])
    B, _, A = pred.shape
    if not (torch.equal(got["best_score"].view(B, A), s) and torch.equal(got["best_cls"].view(B, A).long(), c)):
        return float("inf"), (), "best score / class are not the first maximum of the kernel's own class rows"
    return ratio, idx, note


def judge_nms(i, p, got):
    """i: pred [B, 4 + nc, A] f32 CPU (the GPU's own); got: dict(det, det_idx, det_count) CPU.  Exact against oracle.nms.yolo_nms."""
    from oracle import nms as onms
    want, want_idx = onms.yolo_nms(i["pred"], p["conf"], p["iou"], p["max_det"], return_indices=True)
    for b in range(len(want)):
        n = int(got["det_count"][b])
        if n != want[b].shape[0]:
            return float("inf"), (b,), f"image {b}: {n} detections, the oracle keeps {want[b].shape[0]}"
        if not torch.equal(got["det_idx"][b, :n].long(), want_idx[b]):
            return float("inf"), (b,), f"image {b}: kept anchor indices differ from the oracle's"
        if not torch.equal(got["det"][b, :n], want[b]):
            return float("inf"), (b,), f"image {b}: detection rows differ from the oracle's"
    return 0.0, (), f"{sum(w.shape[0] for w in want)} detections"


JUDGES = {"conv": judge_conv, "c3k2": judge_c3k2, "stem2": judge_stem2, "dwpw": judge_dwpw, "dwconv": judge_dwconv, "sppf_pool": judge_sppf_pool,
          "attention": judge_attention, "decode": judge_decode, "nms": judge_nms}
assert tuple(JUDGES) == KINDS


# ---- outside the view: no byte of any tracked tensor but the launch's output may change ------------------------------------------------------------
class Ledger:
    """Byte images of a set of tensors.  `changed_outside(writes)` compares every tensor with its image and returns a description of the first
    byte that changed outside `writes` -- [(tensor, (c0, c1) channel range of the last dimension, or None for the whole tensor)] -- or None;
    then the images of the written tensors are brought up to date.  Works on either device (the CPU test drives it with plain tensors)."""

    def __init__(self, named):
        self.names, self.tensors = [n for n, _ in named], [t for _, t in named]
        assert all(t.is_contiguous() for t in self.tensors)
        self.sizes = [t.numel() * t.element_size() for t in self.tensors]
        self.offsets = [0]
        for s in self.sizes:
            self.offsets.append(self.offsets[-1] + s)
        self.image = self._bytes()

    def _bytes(self):
        return torch.cat([t.reshape(-1).view(torch.uint8) for t in self.tensors])

    def index_of(self, t):
        for k, x in enumerate(self.tensors):
            if x.data_ptr() == t.data_ptr() and x.numel() == t.numel():
                return k
        raise KeyError("a launch writes a tensor the ledger does not track")

    def changed_outside(self, writes):
        now = self._bytes()
        diff = now != self.image
        for t, chans in writes:
            k = self.index_of(t)
            seg = diff[self.offsets[k]:self.offsets[k + 1]]
            if chans is None:
                seg.zero_()
            else:
                es = t.element_size()
                seg.view(-1, t.shape[-1] * es)[:, chans[0] * es:chans[1] * es] = False
        self.image = now
        if not bool(diff.any()):
            return None
        pos = int(torch.nonzero(diff)[0, 0])
        k = max(j for j in range(len(self.tensors)) if self.offsets[j] <= pos)
        t = self.tensors[k]
        el = (pos - self.offsets[k]) // t.element_size()
        where = tuple(int(v) for v in torch.unravel_index(torch.tensor(el), t.shape))
        return f"{int(diff.sum())} bytes changed outside the output view; first in {self.names[k]}, shape {tuple(t.shape)}, at {where}"


# ---- recording a plan while it is built -----------------------------------------------------------------------------------------------------------
class Recording:
    def __init__(self):
        self.keep_len, self.bufs = [], []


@contextlib.contextmanager
def recording():
    """Wraps Plan.add (notes len(plan.keep) per op) and Buf.__init__ (collects the buffers) for the duration of a plan's construction."""
    from circuitvision_amd import engine
    rec = Recording()
    add0, init0 = engine.Plan.add, engine.Buf.__init__

    def add(self, label, kind, thunk, bytes_=0, flops=0):
        rec.keep_len.append(len(self.keep))
        return add0(self, label, kind, thunk, bytes_, flops)

    def init(self, *a, **kw):
        init0(self, *a, **kw)
        rec.bufs.append(self)

    engine.Plan.add, engine.Buf.__init__ = add, init
    try:
        yield rec
    finally:
        engine.Plan.add, engine.Buf.__init__ = add0, init0


def _closure(thunk, name):
    """A free variable of a launch's thunk: the argument tuple the launch passes."""
    return thunk.__closure__[thunk.__code__.co_freevars.index(name)].cell_contents


def _conv_w(pc):
    return pc.w[:pc.N, :pc.K].view(pc.N, pc.KH, pc.KW, pc.Cin)


def _conv_w_nchw(pc):
    return _conv_w(pc).permute(0, 3, 1, 2).float()


def _view_write(v):
    return (v.buf.t, (v.c0, v.c0 + v.c))


# ---- adapters: keep entry -> (live inputs, parameters, writes, how to read the output) -------------------------------------------------------------
class Launch:
    """One launch under audit.  live: {name: tensor or list of tensors} views of what it reads (snapshotted before it runs); const: weights as
    stored (never written: the ledger tracks them); p: parameters of the judge; writes: the ledger's write list; read(): the output as the
    judge takes it, after the launch."""

    def __init__(self, adapter, live, const, p, writes, read):
        self.adapter, self.live, self.const, self.p, self.writes, self.read = adapter, live, const, p, writes, read


def _adapt_conv(entry, thunk, yp):
    d, pc, srcs, dst, res, row_stats, res_map = entry
    assert isinstance(d, ConvDesc) and row_stats is None and res_map is None and not d.shuffle_cout and not d.res_mod and d.res_rep <= 1
    assert (d.KH, d.KW, d.N, d.B) == (pc.KH, pc.KW, pc.N, dst.B)
    # the descriptor the launch reads names these very operands
    assert (d.x0, d.x0_ld, d.c0, d.y, d.y_ld, d.w, d.bias) == (srcs[0][0].ptr, srcs[0][0].ld, srcs[0][0].c, dst.ptr, dst.ld, pc.w.data_ptr(), pc.bias.data_ptr())
    assert (d.x1 or 0, d.c1) == ((srcs[1][0].ptr, srcs[1][0].c) if len(srcs) > 1 else (0, 0)) and (d.res or 0) == (res.ptr if res is not None else 0)
    live = dict(srcs=[v.tensor() for v, _ in srcs])
    if res is not None:
        live["res"] = res.tensor()
    p = dict(stride=d.stride, pad=d.pad, OH=d.OH, OW=d.OW, ups=[up for _, up in srcs], act=d.act, act_after_res=d.act_after_res,
             out=dst.tensor().dtype, fast=pc.dtype != F32)
    return Launch("conv", live, dict(w=_conv_w(pc), bias=pc.bias[:pc.N]), p, [_view_write(dst)], lambda: dst.tensor().clone())


def _adapt_c3k2(entry, thunk, yp):
    d, src, dst, pc0, pc1, pc2, pc3 = entry
    assert isinstance(d, C3k2Desc) and d.dtype == F16 and (d.x, d.x_ld, d.y, d.y_ld, d.w3) == (src.ptr, src.ld, dst.ptr, dst.ld, pc3.w.data_ptr())
    const = dict(w0=None, b0=None, w1=_conv_w_nchw(pc1), b1=pc1.bias[:pc1.N], w2=_conv_w_nchw(pc2), b2=pc2.bias[:pc2.N], w3=_conv_w_nchw(pc3), b3=pc3.bias[:pc3.N])
    if d.fuse_cv1:
        const.update(w0=_conv_w_nchw(pc0), b0=pc0.bias[:pc0.N])
    return Launch("c3k2", dict(x=src.tensor()), const, dict(shortcut=bool(d.shortcut), fuse_cv1=bool(d.fuse_cv1)), [_view_write(dst)],
                  lambda: dst.tensor().clone())


def _adapt_stem2(entry, thunk, yp):
    pc0, pc1, src, dst = entry
    args = _closure(thunk, "args")
    assert pc1.dtype == F16 and (args[0], args[1], args[2], args[8], args[9]) == (src.ptr, src.ld, pc0.w.data_ptr(), dst.ptr, dst.ld)
    const = dict(w0=_conv_w_nchw(pc0), b0=pc0.bias[:pc0.N], w1=_conv_w_nchw(pc1), b1=pc1.bias[:pc1.N])
    return Launch("stem2", dict(x=src.tensor()), const, {}, [_view_write(dst)], lambda: dst.tensor().clone())


def _adapt_dwpw(entry, thunk, yp):
    d, pd, pc1, pc2, src, dst = entry
    assert isinstance(d, DwPwDesc) and d.dtype == F16 and (d.x, d.x_ld, d.y, d.y_ld, d.wd) == (src.ptr, src.ld, dst.ptr, dst.ld, pd.w.data_ptr())
    const = dict(wd=pd.w.t().reshape(pd.C, 1, 3, 3).float(), bd=pd.bias, w1=_conv_w_nchw(pc1), b1=pc1.bias[:pc1.N])
    if pc2 is not None:
        const.update(w2=_conv_w_nchw(pc2), b2=pc2.bias[:pc2.N])
    return Launch("dwpw", dict(x=src.tensor()), const, {}, [_view_write(dst)], lambda: dst.tensor().clone())


def _adapt_dwconv(entry, thunk, yp):
    pd, src, dst, res = entry
    args = _closure(thunk, "args")
    act = args[12]
    assert act in (ACT_NONE, ACT_SILU), act
    assert (args[0], args[1], args[2], args[4], args[6], args[7]) == (src.ptr, src.ld, pd.w.data_ptr(), res.ptr if res is not None else None, dst.ptr, dst.ld)
    live = dict(x=src.tensor())
    if res is not None:
        live["res"] = res.tensor()
    p = dict(act="silu" if act == ACT_SILU else "none", stored=STORED[dst.tensor().dtype])
    return Launch("dwconv", live, dict(w=pd.w.t().reshape(pd.C, 1, 3, 3).float(), b=pd.bias), p, [_view_write(dst)], lambda: dst.tensor().clone())


def _adapt_sppf_pool(entry, thunk, yp):
    buf = entry
    args = _closure(thunk, "args")
    c = args[5]
    assert buf.C == 4 * c and (args[0], args[1]) == (buf.t.data_ptr(), buf.C)
    return Launch("sppf_pool", dict(x=buf.t[..., :c]), {}, {}, [(buf.t, (c, 4 * c))], lambda: buf.t[..., c:].clone())


def _adapt_attention(entry, thunk, yp):
    d, (QKV, AO) = entry
    assert isinstance(d, AttnDesc) and not (d.win or d.q_pool or d.q_bdiv or d.kv_bdiv or d.av_fp8 or d.q_log2 or d.proj_x)
    es = QKV.t.element_size()
    B, N, nh, per, kd, hd = d.B, d.Nq, d.heads, d.q_sh, d.dqk, d.dv
    assert d.q == QKV.t.data_ptr() and d.k == d.q + kd * es and d.v == d.q + 2 * kd * es and d.o == AO.t.data_ptr() and d.Nk == N
    assert (d.q_st, d.k_st, d.v_st, d.o_st, d.o_sh) == (QKV.C, QKV.C, QKV.C, AO.C, hd) and d.k_sh == per and d.v_sh == per and nh * per == QKV.C
    assert (d.q_sb, d.o_sb) == (N * QKV.C, N * AO.C) and QKV.t.numel() == B * N * QKV.C and nh * hd == AO.C

    def heads(t, lo, n):                                   # [B, H, W, heads * per] -> [B, heads, N, n]
        return t.reshape(B, N, nh, per)[..., lo:lo + n].permute(0, 2, 1, 3)

    live = dict(qkv=QKV.t)
    p = dict(scale=float(d.scale), out=AO.t.dtype, split=lambda t: dict(q=heads(t, 0, kd), k=heads(t, kd, kd), v=heads(t, 2 * kd, hd)))
    return Launch("attention", live, {}, p, [(AO.t, None)], lambda: AO.t.reshape(B, N, nh, hd).permute(0, 2, 1, 3).clone())


def _adapt_decode(entry, thunk, yp):
    nc = yp.wt.nc
    live = dict(box=[b.tensor() for b in yp.box_bufs], cls=[c.t[..., :nc] for c in yp.cls_bufs])
    assert yp.keep_scores and [int(yp.H // b.H) for b in yp.box_bufs] == [8, 16, 32]
    writes = [(yp.pred, None), (yp.best_score, None), (yp.best_cls, None)]
    return Launch("decode", live, {}, dict(nc=nc), writes, lambda: dict(pred=yp.pred.cpu(), best_score=yp.best_score.cpu(), best_cls=yp.best_cls.cpu()))


def _adapt_nms(entry, thunk, yp):
    writes = [(yp.det, None), (yp.det_idx, None), (yp.det_count, None)]
    return Launch("nms", dict(pred=yp.pred), {}, dict(conf=yp.conf, iou=yp.iou, max_det=yp.max_det), writes,
                  lambda: dict(det=yp.det.cpu(), det_idx=yp.det_idx.cpu(), det_count=yp.det_count.cpu()))


ADAPTERS = {"conv": _adapt_conv, "c3k2": _adapt_c3k2, "stem2": _adapt_stem2, "dwpw": _adapt_dwpw, "dwconv": _adapt_dwconv,
            "sppf_pool": _adapt_sppf_pool, "attention": _adapt_attention, "decode": _adapt_decode, "nms": _adapt_nms}
assert tuple(ADAPTERS) == KINDS


def _snapshot(live, to_cpu):
    def one(t):
        t = t.detach().clone(memory_format=torch.contiguous_format)
        return t.float().cpu() if to_cpu else t
    return {k: [one(t) for t in v] if isinstance(v, list) else one(v) for k, v in live.items()}


def judge_launch(launch, snap, got):
    """The judge's inputs from a snapshot of the live views plus the stored weights, then the judge."""
    i = dict(snap)
    i.update(launch.const)
    if launch.adapter == "attention":
        i = launch.p["split"](snap["qkv"])
    elif launch.adapter == "decode":
        i = dict(levels=list(zip(snap["box"], snap["cls"])))
    return JUDGES[launch.adapter](i, launch.p, got)


# ---- the stepper --------------------------------------------------------------------------------------------------------------------------------
def tracked_tensors(yp, rec):
    """Everything the plan owns that a launch could damage: every Buf built with the plan, the packed weights, and the tail's tensors.  The NMS
    workspace is scratch of that one launch and is not tracked."""
    named = [(f"buffer {k}", b.t) for k, b in enumerate(rec.bufs)]
    for key, pk in yp.wt.packed.items():
        named += [(f"weight {key}", pk.w), (f"bias {key}", pk.bias)]
    named += [(n, getattr(yp, n)) for n in ("pred", "best_score", "best_cls", "det", "det_idx", "det_count") if hasattr(yp, n)]
    return named


def audit(yp, rec, case_id="", ledger_all=True):
    """Runs the plan launch by launch on whatever input it holds.  Returns (results, failures): results = [dict(label, kind, adapter, kernel,
    ratio, seconds)] for every judged launch; failures = lines `label, kind, kernel tag, worst ratio, worst element (b, y, x, c)`.
    ledger_all=False restricts the outside-the-view check to the launch's own output tensors."""
    from circuitvision_amd import _lib
    lib = _lib.load()
    ops = yp.plan.ops
    assert len(rec.keep_len) == len(ops)
    named = tracked_tensors(yp, rec)
    torch.cuda.synchronize()
    ledger = Ledger(named) if ledger_all else None
    results, failures = [], []
    for (label, kind, thunk, _, _), klen in zip(ops, rec.keep_len):
        adapter = resolve(label, kind, yp.route)
        if adapter is None:
            continue
        t0 = time.time()
        entry = yp.plan.keep[klen - 1] if adapter not in ("decode", "nms") else None
        launch = ADAPTERS[adapter](entry, thunk, yp)
        snap = _snapshot(launch.live, to_cpu=adapter in ("decode", "nms"))
        if not ledger_all:
            ledger = Ledger([(n, t) for n, t in named if any(t.data_ptr() == w.data_ptr() for w, _ in launch.writes)])
        lib.cvmi_last_kernel()                                              # clears the tag
        torch.cuda.synchronize()
        thunk()
        torch.cuda.synchronize()
        tag = lib.cvmi_last_kernel().decode()
        got = launch.read()
        ratio, idx, note = judge_launch(launch, snap, got)
        ratio /= RELAX.get((case_id, label), 1.0)
        damage = ledger.changed_outside(launch.writes)
        if not kernel_fits(adapter, tag):
            failures.append(f"{label}, {kind}, {tag!r}: the kernel tag does not belong to the {adapter} adapter")
        if not ratio <= 1.0:
            failures.append(f"{label}, {kind}, {tag!r}, err/bound {ratio:.3f}, worst element {idx}: {note}")
        if damage:
            failures.append(f"{label}, {kind}, {tag!r}: {damage}")
        results.append(dict(label=label, kind=kind, adapter=adapter, kernel=tag, ratio=ratio, seconds=time.time() - t0))
    return results, failures


def summary(results):
    """{adapter: (launches judged, worst ratio)}."""
    out = {}
    for r in results:
        n, w = out.get(r["adapter"], (0, 0.0))
        out[r["adapter"]] = (n + 1, max(w, r["ratio"]))
    return out
