"""YOLO11 detector on the cvmi355 kernels: weight packing + launch plan.

What it replaces: the network behind `self.yolo.predict(image)` in the reference
(/root/reference/src/circuit_analyzer.py:45, :268; architecture from un-vendored ultralytics,
SURVEY.md section 8 Table Y).  Parameters are addressed by ultralytics' own state_dict keys
(`model.2.m.0.cv1.conv.weight`, `model.2.m.0.cv1.bn.running_var`, ...), so a real checkpoint's
tensors drop in; BatchNorm is folded into the conv at pack time.

Design notes (MI355X):
  * activations NHWC fp16 (or f32 in parity mode); every Conv+BN+SiLU is ONE implicit-GEMM launch
  * Upsample / Concat / chunk are never materialised: convs read two channel-concatenated,
    optionally 2x-upsampled sources and write into channel slices of the consumer's buffer
  * C3k's parallel cv1/cv2 1x1 convs are one launch (weights stacked along Cout)
  * the whole forward + decode + NMS is captured once per input shape into a HIP graph
  * the network itself, and which launches a plan takes, are stated in yolo_route.py: the weights pack what its table names,
    the plan wires buffers over the same table and emits what the route says
"""
import hashlib
import math

import torch

from . import _lib
from ._lib import ACT_NONE, ACT_SILU, F16
from .engine import ESIZE, Buf, PackedConv, PackedDW, Plan, make_attn_desc, op_attention, op_c3k2, op_conv, op_dwconv, op_dwpw, op_sppf_pool, op_stem2
from .yolo_route import (PSA_HD, YoloSwitches, c2psa_geometry, c3k2_widths, detect_geometry, layer_convs, route_yolo, scale_fns, yolo_lanes,
                         yolo_layers, yolo_switches)

BN_EPS = 1e-3


# ---- parameter sources ---------------------------------------------------------------------------
class SyntheticParams:
    """Seeded synthetic weights; records everything it hands out so that
    `state_dict()` is a complete ultralytics-keyed checkpoint for the oracle to load."""

    def __init__(self, seed=0, nc=62):
        self.seed, self.nc, self.sd = seed, nc, {}

    def _gen(self, name):
        h = int.from_bytes(hashlib.sha256(f"{self.seed}:{name}".encode()).digest()[:8], "little") & 0x7FFFFFFFFFFFFFFF
        return torch.Generator().manual_seed(h)

    def get(self, name, shape):
        if name in self.sd:
            assert tuple(self.sd[name].shape) == tuple(shape), name
            return self.sd[name]
        g = self._gen(name)
        leaf = name.rsplit(".", 1)[-1]
        if name.endswith("bn.weight"):
            t = torch.empty(shape).uniform_(0.5, 1.5, generator=g)
        elif name.endswith("bn.bias") or name.endswith("bn.running_mean"):
            t = torch.empty(shape).normal_(0, 0.1, generator=g)
        elif name.endswith("bn.running_var"):
            t = torch.empty(shape).uniform_(0.5, 1.5, generator=g)
        elif name.endswith("num_batches_tracked"):
            t = torch.zeros(shape, dtype=torch.long)
        elif leaf == "weight":
            fan_in = shape[1] * shape[2] * shape[3]
            t = torch.empty(shape).uniform_(-1, 1, generator=g) * (1.0 / math.sqrt(fan_in))
            if ".cv3." in name and name.endswith(".2.weight"):       # class logits: spread them out
                t = t * 6.0
        elif leaf == "bias":
            if ".cv3." in name:                                          # sparse detections (~1-3 % of anchors)
                t = torch.empty(shape).normal_(-6.0, 0.5, generator=g)
            else:
                t = torch.empty(shape).normal_(1.0, 0.5, generator=g)    # DFL logits bias
        else:
            raise KeyError(name)
        self.sd[name] = t
        return t

    def state_dict(self):
        return dict(self.sd)


class BlankParams:
    """A rank that holds NO checkpoint: every tensor reads as zeros (BatchNorm variance one), so the packed buffers get their final
    shapes and the real values arrive by `distributed.broadcast_packed` from the rank that read the checkpoint."""

    def get(self, name, shape):
        if name.endswith("num_batches_tracked"):
            return torch.zeros(shape, dtype=torch.long)
        return torch.ones(shape) if name.endswith("running_var") else torch.zeros(shape)


class StateDictParams:
    def __init__(self, sd):
        self.sd = sd

    def get(self, name, shape):
        t = self.sd[name]
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name}: checkpoint shape {tuple(t.shape)} != expected {tuple(shape)}")
        return t.detach().float().cpu()


# ---- packed model ----------------------------------------------------------------------------------
class Yolo11Weights:
    """Walks the YOLO11 table (yolo_route.yolo_layers) once, pulling every parameter from `params` and packing it."""

    def __init__(self, scale, nc, params, dtype=F16, device="cuda"):
        self.scale, self.nc, self.dtype, self.device = scale, nc, dtype, device
        self.p = params
        self.ch, self.rep = scale_fns(scale)
        self.layers = yolo_layers(scale, nc)
        g = detect_geometry(self.layers[-1])
        self.det_ch, self.det_c2, self.det_c3 = g.ch, g.c2, g.c3
        self.packed = {}
        self.param_bytes = 0
        for L in self.layers:
            for spec in layer_convs(L):
                getattr(self, "_" + spec.form)(spec)                 # one packer per ConvSpec.form
        if isinstance(self.p, SyntheticParams):
            self.p.sd[f"{self.layers[-1].name}.dfl.conv.weight"] = torch.arange(16, dtype=torch.float32).view(1, 16, 1, 1)

    def _fold(self, name, c1, c2, k, g=1):
        w = self.p.get(f"{name}.conv.weight", (c2, c1 // g, k, k))
        gamma = self.p.get(f"{name}.bn.weight", (c2,))
        beta = self.p.get(f"{name}.bn.bias", (c2,))
        mean = self.p.get(f"{name}.bn.running_mean", (c2,))
        var = self.p.get(f"{name}.bn.running_var", (c2,))
        self.p.get(f"{name}.bn.num_batches_tracked", ()) if isinstance(self.p, SyntheticParams) else None
        s = gamma / torch.sqrt(var + BN_EPS)
        return w * s.view(-1, 1, 1, 1), beta - mean * s

    def _add(self, key, packed):
        self.packed[key] = packed
        self.param_bytes += packed.param_bytes

    def _conv(self, s):
        w, b = self._fold(s.key, s.c1, s.c2, s.k)
        self._add(s.key, PackedConv(w, b, self.dtype, self.device))

    def _pair(self, s):
        """`...cv12`: the cv1 and cv2 of a C3k, stacked along Cout."""
        wa, ba = self._fold(s.key[:-1], s.c1, s.c2, s.k)
        wb, bb = self._fold(s.key[:-2] + "2", s.c1, s.c2, s.k)
        self._add(s.key, PackedConv(torch.cat((wa, wb), 0), torch.cat((ba, bb), 0), self.dtype, self.device))

    def _dw(self, s):
        w, b = self._fold(s.key, s.c1, s.c2, s.k, g=s.c2)
        self._add(s.key, PackedDW(w, b, self.dtype, self.device))

    def _dw_heads(self, s):
        """C2PSA's positional depthwise conv acts on v, one hd-channel group per head."""
        w, b = self._fold(s.key, s.c1, s.c2, s.k, g=s.c2)
        hd = PSA_HD
        for h in range(s.c2 // hd):                                  # (c2psa_geometry: c2 = heads * hd)
            self._add(f"{s.key}.h{h}", PackedDW(w[h * hd:(h + 1) * hd], b[h * hd:(h + 1) * hd], self.dtype, self.device))

    def _plain(self, s):
        w = self.p.get(f"{s.key}.weight", (s.c2, s.c1, s.k, s.k))
        b = self.p.get(f"{s.key}.bias", (s.c2,))
        self._add(s.key, PackedConv(w, b, self.dtype, self.device))

    def _stem(self, s):
        """Layer 0 (3x3, stride 2, 3 channels) re-expressed on the space-to-depth(2) input the letterbox kernel writes:
        a 2x2 / stride-1 conv over 16 channels (12 real), taps (ty, tx) = block offsets (-1, 0).  Window row ky sits in
        block row ty with sub-row sy: ky=0 -> (0,1), ky=1 -> (1,0), ky=2 -> (1,1); same for columns."""
        w, b = self._fold(s.key, s.c1, s.c2, s.k)
        w2 = torch.zeros(s.c2, 16, 2, 2)
        m = {0: (0, 1), 1: (1, 0), 2: (1, 1)}
        for ky in range(3):
            for kx in range(3):
                (ty, sy), (tx, sx) = m[ky], m[kx]
                w2[:, (sy * 2 + sx) * 3:(sy * 2 + sx) * 3 + 3, ty, tx] = w[:, :, ky, kx]
        self._add(s.key, PackedConv(w2, b, self.dtype, self.device))


class Yolo11Plan:
    """Launch plan of the full forward for one (B, H, W): input NHWC [B,H,W,3] -> pred f32 [B,4+nc,A]
    -> NMS outputs.  `self.route` (yolo_route.route_yolo) says which launches; the methods below say over which buffers."""

    def __init__(self, weights, B, H, W, stream, conf=0.25, iou=0.7, max_det=300, with_nms=True, keep_scores=True, fuse_c3k2=True, lanes=None):
        """keep_scores=False: the decode kernel skips the class-score rows of `pred` (NMS takes the per-anchor
        best class straight from the decode kernel); the detections are identical.  fuse_c3k2=False: every fused launch off,
        as with all three CVMI_FUSE_* switches at "0".  lanes: a yolo_route.LANE_MODES mode (None: CVMI_YOLO_LANES)."""
        self.keep_scores = keep_scores
        assert H % 32 == 0 and W % 32 == 0, "network input must be a multiple of stride 32"
        self.wt, self.B, self.H, self.W = weights, B, H, W
        self.dt, self.dev = weights.dtype, weights.device
        self.sw = yolo_switches() if fuse_c3k2 else YoloSwitches(*(False,) * len(YoloSwitches._fields))
        self.lanes = yolo_lanes() if lanes is None else int(lanes)      # side lanes of the captured graph
        self.route = route_yolo(weights.scale, weights.nc, self.dt, self.sw, self.lanes)
        self.plan = Plan(stream)
        self.act_bytes = 0
        self.conf, self.iou, self.max_det = conf, iou, max_det
        self._build(with_nms)
        torch.cuda.synchronize()      # buffer fills / weight uploads ran on the default stream

    # -- helpers
    def buf(self, H, W, C):
        b = Buf(self.B, H, W, C, self.dt, self.dev)
        self.act_bytes += b.nbytes
        return b

    def cv(self, name, srcs, dst, s=1, act=ACT_SILU, res=None, kind="conv"):
        if not isinstance(srcs, list):
            srcs = [(srcs, 0)]
        op_conv(self.plan, name, self.wt.packed[name], srcs, dst, stride=s, act=act, res=res, kind=kind)

    def _build(self, with_nms):
        layers = self.route.layers
        det = layers[-1]
        level_of = {s: i for i, (s, _) in enumerate(det.srcs)}
        self.x_in = Buf(self.B, self.H // 2, self.W // 2, 16, self.dt, self.dev, zero=True)       # space-to-depth(2) image, see Yolo11Weights._stem
        self._det_boxes, self._det_cls = [], []
        out = {}
        for L in layers[:-1]:
            out[L.name] = getattr(self, "_" + L.op)(L, [(out[s], up) for s, up in L.srcs])
            if L.name in level_of:            # a Detect level starts as soon as its feature map exists (yolo_route.LANE_MODES)
                self._detect_level(det, level_of[L.name], out[L.name])
        self.feats = tuple(out[s] for s, _ in det.srcs)
        self._detect(list(self.feats), with_nms)

    # -- one emitter per Layer.op: (layer, [(source view, upsample)]) -> output view
    def _stem(self, L, srcs):
        return self.x_in.view()               # launched by its consumer (`_conv`): one launch for both layers when the route fuses them

    def _conv(self, L, srcs):
        (v, _), = srcs
        pk = self.wt.packed
        y = self.buf(v.H // L.s, v.W // L.s, L.c2).view()
        if v.buf is not self.x_in:
            self.cv(L.name, v, y, L.s)
        elif self.route.stem == "fused":
            op_stem2(self.plan, "model.0-1", pk["model.0"], pk[L.name], v, y)
        else:
            x = self.buf(v.H, v.W, pk["model.0"].N).view()
            op_conv(self.plan, "model.0", pk["model.0"], [(v, 0)], x, stride=1, pad=1, act=ACT_SILU, out_hw=(v.H, v.W), kind="stem")
            self.cv(L.name, x, y, L.s)
        return y

    def bottleneck(self, name, src, dst):
        t = self.buf(src.H, src.W, self.wt.packed[f"{name}.cv1"].N).view()
        self.cv(f"{name}.cv1", src, t)
        self.cv(f"{name}.cv2", t, dst, res=src)

    def c3k(self, name, src, dst):
        c_ = self.wt.packed[f"{name}.cv12"].N // 2
        Z = self.buf(src.H, src.W, 2 * c_)
        self.cv(f"{name}.cv12", src, Z.view())
        t = self.buf(src.H, src.W, c_).view()
        self.bottleneck(f"{name}.m.0", Z.view(0, c_), t)
        self.bottleneck(f"{name}.m.1", t, Z.view(0, c_))
        self.cv(f"{name}.cv3", Z.view(), dst)

    def _c3k2(self, L, srcs):
        name, pk, mode = L.name, self.wt.packed, self.route.c3k2[L.name]
        v0, up0 = srcs[0]
        H, W = v0.H << up0, v0.W << up0
        c, h = c3k2_widths(L)
        dst = self.buf(H, W, L.c2).view()
        if mode != "chain":
            args = (pk[f"{name}.cv1"], pk[f"{name}.m.0.cv1"], pk[f"{name}.m.0.cv2"], pk[f"{name}.cv2"], c, h)
            if mode == "fused_cv1":
                op_c3k2(self.plan, name, v0, dst, *args, fuse_cv1=True)
            else:
                Y = self.buf(H, W, 2 * c)
                self.cv(f"{name}.cv1", srcs, Y.view())
                op_c3k2(self.plan, f"{name}.fused", Y.view(), dst, *args, fuse_cv1=False)
            return dst
        Y = self.buf(H, W, (2 + L.n) * c)
        self.cv(f"{name}.cv1", srcs, Y.view(0, 2 * c))
        for i in range(L.n):
            (self.c3k if L.c3k else self.bottleneck)(f"{name}.m.{i}", Y.view((1 + i) * c, c), Y.view((2 + i) * c, c))
        self.cv(f"{name}.cv2", Y.view(), dst)
        return dst

    def _sppf(self, L, srcs):
        (x, _), = srcs
        c_ = L.c1 // 2
        S = self.buf(x.H, x.W, 4 * c_)
        self.cv(f"{L.name}.cv1", x, S.view(0, c_))
        op_sppf_pool(self.plan, f"{L.name}.pool", S, c_)
        y = self.buf(x.H, x.W, L.c2).view()
        self.cv(f"{L.name}.cv2", S.view(), y)
        return y

    def _c2psa(self, L, srcs):
        (x, _), = srcs
        name = L.name
        cp, nh, kd, hd, per, _ = c2psa_geometry(L)
        Hh, Ww = x.H, x.W
        N = Hh * Ww
        Y = self.buf(Hh, Ww, 2 * cp)
        self.cv(f"{name}.cv1", x, Y.view())
        b = Y.view(cp, cp)
        for i in range(L.n):
            a = f"{name}.m.{i}.attn"
            QKV = self.buf(Hh, Ww, nh * per)
            self.cv(f"{a}.qkv", b, QKV.view(), act=ACT_NONE)
            AO = self.buf(Hh, Ww, cp)
            es = ESIZE[self.dt]
            base = QKV.t.data_ptr()
            desc = make_attn_desc(
                q=base, k=base + kd * es, v=base + 2 * kd * es, o=AO.t.data_ptr(),
                q_sb=N * QKV.C, q_sh=per, q_st=QKV.C, k_sb=N * QKV.C, k_sh=per, k_st=QKV.C,
                v_sb=N * QKV.C, v_sh=per, v_st=QKV.C, o_sb=N * cp, o_sh=hd, o_st=cp,
                B=self.B, heads=nh, Nq=N, Nk=N, dqk=kd, dv=hd, scale=kd ** -0.5, dtype=self.dt,
                win=0, grid_h=0, grid_w=0, q_pool=0)
            op_attention(self.plan, f"{a}.sdpa", desc, (QKV, AO), bytes_=(QKV.nbytes + AO.nbytes),
                         flops=2 * self.B * nh * N * N * (kd + hd))
            for h in range(nh):
                op_dwconv(self.plan, f"{a}.pe.h{h}", self.wt.packed[f"{a}.pe.h{h}"], QKV.view(h * per + 2 * kd, hd),
                          AO.view(h * hd, hd), act=ACT_NONE, res=AO.view(h * hd, hd))
            self.cv(f"{a}.proj", AO.view(), b, act=ACT_NONE, res=b)
            F = self.buf(Hh, Ww, 2 * cp)
            self.cv(f"{name}.m.{i}.ffn.0", b, F.view())
            self.cv(f"{name}.m.{i}.ffn.1", F.view(), b, act=ACT_NONE, res=b)
        out = self.buf(Hh, Ww, L.c2).view()
        self.cv(f"{name}.cv2", Y.view(), out)
        return out

    def _detect_level(self, det, i, f):
        """Detect branches of level i (box: 3x3, 3x3, 1x1; cls: dw3x3 + 1x1 twice, 1x1) on the route's side lanes."""
        pk, nc, lanes = self.wt.packed, det.c2, self.route.lanes
        _, c2, c3, ncp = detect_geometry(det)
        bxn, cln = f"{det.name}.cv2.{i}", f"{det.name}.cv3.{i}"
        if lanes:
            self.plan.fork()
            self.plan.lane(lanes[i][0])
        t1 = self.buf(f.H, f.W, c2).view()
        t2 = self.buf(f.H, f.W, c2).view()
        bx = self.buf(f.H, f.W, 64).view()
        self.cv(f"{bxn}.0", f, t1, kind="head")
        self.cv(f"{bxn}.1", t1, t2, kind="head")
        self.cv(f"{bxn}.2", t2, bx, act=ACT_NONE, kind="head")
        if lanes:
            self.plan.lane(lanes[i][1])
        cl = Buf(self.B, f.H, f.W, ncp, self.dt, self.dev, zero=True)
        self.act_bytes += cl.nbytes
        u1 = self.buf(f.H, f.W, c3).view()
        if self.route.cls[i] == "dwpw":
            # class branch in two launches: [dw3x3 + 1x1], [dw3x3 + 1x1 + class 1x1]; the intermediates stay in LDS
            op_dwpw(self.plan, f"{cln}.0", pk[f"{cln}.0.0"], pk[f"{cln}.0.1"], f, u1)
            op_dwpw(self.plan, f"{cln}.1-2", pk[f"{cln}.1.0"], pk[f"{cln}.1.1"], u1, cl.view(0, nc), pc2=pk[f"{cln}.2"])
        else:
            d1 = self.buf(f.H, f.W, f.c).view()
            op_dwconv(self.plan, f"{cln}.0.0", pk[f"{cln}.0.0"], f, d1, act=ACT_SILU)
            self.cv(f"{cln}.0.1", d1, u1, kind="head")
            d2 = self.buf(f.H, f.W, c3).view()
            op_dwconv(self.plan, f"{cln}.1.0", pk[f"{cln}.1.0"], u1, d2, act=ACT_SILU)
            u2 = self.buf(f.H, f.W, c3).view()
            self.cv(f"{cln}.1.1", d2, u2, kind="head")
            self.cv(f"{cln}.2", u2, cl.view(0, nc), act=ACT_NONE, kind="head")
        self._det_boxes.append(bx)
        self._det_cls.append(cl)
        self.plan.lane(0)

    def _detect(self, feats, with_nms):
        import ctypes as C
        wt, lib = self.wt, _lib.load()
        nc = wt.nc
        boxes, clss = self._det_boxes, self._det_cls
        self.plan.join()
        self.box_bufs, self.cls_bufs = boxes, clss
        A = sum(f.H * f.W for f in feats)
        self.A = A
        self.pred = torch.empty(self.B, 4 + nc, A, dtype=torch.float32, device=self.dev)
        nl = len(feats)
        box_p = (C.c_void_p * nl)(*[b.ptr for b in boxes])
        cls_p = (C.c_void_p * nl)(*[c.t.data_ptr() for c in clss])
        box_ld = (C.c_int * nl)(*[b.ld for b in boxes])
        cls_ld = (C.c_int * nl)(*[c.C for c in clss])
        hs = (C.c_int * nl)(*[f.H for f in feats])
        ws = (C.c_int * nl)(*[f.W for f in feats])
        strides = (C.c_float * nl)(*[float(self.H // f.H) for f in feats])
        self.plan.keep.append((box_p, cls_p, box_ld, cls_ld, hs, ws, strides))
        sp, dt, pred_ptr, Bn = self.plan.sptr, self.dt, self.pred.data_ptr(), self.B
        self.best_score = torch.zeros(Bn * A, dtype=torch.float32, device=self.dev)
        self.best_cls = torch.zeros(Bn * A, dtype=torch.int32, device=self.dev)
        bs_ptr, bc_ptr, wcls = self.best_score.data_ptr(), self.best_cls.data_ptr(), 1 if self.keep_scores else 0
        if not self.keep_scores:
            self.pred.zero_()

        def decode(sp=sp):
            _lib.check(lib.cvmi_detect_decode(box_p, box_ld, cls_p, cls_ld, hs, ws, strides, nl, Bn, nc, dt, pred_ptr, bs_ptr, bc_ptr, wcls, sp), "detect_decode")

        es = ESIZE[self.dt]
        self.plan.add("model.23.decode", "decode", decode, Bn * A * ((64 + nc) * es + (4 + (nc if wcls else 2)) * 4), 0)
        if with_nms:
            self.det = torch.zeros(Bn, self.max_det, 6, dtype=torch.float32, device=self.dev)
            self.det_idx = torch.zeros(Bn, self.max_det, dtype=torch.int32, device=self.dev)
            self.det_count = torch.zeros(Bn, dtype=torch.int32, device=self.dev)
            self.nms_ws = torch.empty(lib.cvmi_yolo_nms_workspace(Bn, A), dtype=torch.uint8, device=self.dev)
            a = (pred_ptr, bs_ptr, bc_ptr, Bn, nc, A, float(self.conf), float(self.iou), int(self.max_det), 7680.0, self.det.data_ptr(),
                 self.det_idx.data_ptr(), self.det_count.data_ptr(), self.nms_ws.data_ptr())

            def nms(sp=sp):
                _lib.check(lib.cvmi_yolo_nms_best(*a, sp), "yolo_nms")

            self.plan.add("nms", "nms", nms, Bn * A * 6 * 4, 0)

    def set_input_nchw(self, x):
        """x: [B,3,H,W] float tensor (already letterboxed, RGB-flipped, /255) -> the plan's space-to-depth input."""
        B, _, H, W = x.shape
        t = x.to(self.dev).reshape(B, 3, H // 2, 2, W // 2, 2).permute(0, 2, 4, 3, 5, 1).reshape(B, H // 2, W // 2, 12)
        self.x_in.t.zero_()
        self.x_in.t[..., :12] = t.to(self.x_in.t.dtype)

    def input_nchw(self):
        B, H2, W2, _ = self.x_in.t.shape
        t = self.x_in.t[..., :12].float().reshape(B, H2, W2, 2, 2, 3).permute(0, 5, 1, 3, 2, 4).reshape(B, 3, H2 * 2, W2 * 2)
        return t

    # -- accounting for the roofline line (layer-granular minimum traffic)
    def conv_stack_bytes(self):
        return sum(b for _, kind, _, b, _ in self.plan.ops if kind in ("conv", "stem", "head", "dwconv", "pool", "attention"))

    def flops(self):
        return sum(f for *_, f in self.plan.ops)
