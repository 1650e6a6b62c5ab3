"""YOLO11 stated once, and which launches a detector plan takes, decided apart from emitting them, in the manner of hiera_route.py: the
`CVMI_FUSE_*` switches and `CVMI_YOLO_LANES`, the network as a table of layers (`yolo_layers`), the convolutions each layer owns (`layer_convs`),
the side lanes of the Detect heads (`LANE_MODES`) and the `YoloRoute` of one (scale, classes, dtype, switches, lane mode).  Everything here is a
pure function -- no device, no buffers, no tensors -- so any configuration can be read (and is tested, tests/test_yolo_route_cpu.py) without a GPU.
`yolo11.Yolo11Weights` packs what `layer_convs` names; `yolo11.Yolo11Plan` wires buffers over the same table and emits what `route_yolo` returns."""
import math
import os
from typing import NamedTuple, Optional

from .engine import c3k2_supported, dwpw_supported, stem2_supported

# field -> (environment variable, who reads it, what "0" restores); every switch defaults to "1", read when a plan is built
SWITCH_TABLE = dict(
    fuse_c3k2=("CVMI_FUSE_C3K2", "plan", "every C3k2 block as its chain of conv launches (no c3k2 kernel)"),
    fuse_dwpw=("CVMI_FUSE_DWPW", "plan", "each Detect class branch as five launches: dw3x3, 1x1, dw3x3, 1x1, 1x1 (no dwpw kernel)"),
    fuse_stem=("CVMI_FUSE_STEM", "plan", "model.0 and model.1 as two conv launches (no stem2 kernel)"),
)
YoloSwitches = NamedTuple("YoloSwitches", [(f, bool) for f in SWITCH_TABLE])      # one bool per row of the table, True = on
LANES_VARIABLE = "CVMI_YOLO_LANES"

# Side lanes of the captured graph: the (box lane, class lane) of Detect level i, per mode.  Each Detect level is forked onto side lanes as soon as
# its feature map exists, so the long 80 x 80 chains run beside model.17 .. model.22 (small grids that leave most CUs idle) instead of after them.
# Measured (B = 32, ms per step): every branch on its own lane (6 lanes) 1.16, one lane per level 1.10, ONE side lane for all heads 1.09, no side
# lane 1.16 -- a replayed HIP graph pays ~1.8 us per node on a chain but ~3.3 us per node when nodes alternate between lanes (tools/graph_gap.py),
# so the heads share one lane that runs beside the rest of the neck.  CVMI_YOLO_LANES: tuning experiments only; a plan's default is mode 3.
# (Yolo11Plan(lanes=0): one linear chain -- for a step whose graphs run side by side on their own streams)
LANE_MODES = {
    0: ("no fork, one chain", None),
    1: ("one lane per level", ((1, 1), (3, 3), (5, 5))),
    2: ("one lane per branch", ((1, 2), (3, 4), (5, 6))),
    3: ("one side lane for all heads", ((1, 1), (1, 1), (1, 1))),
    4: ("level 0 on lane 1, levels 1-2 on lane 2", ((1, 1), (2, 2), (2, 2))),
    5: ("as mode 3, but the last level's class branch on lane 2 (the serial tail of the step: its two branches side by side)", ((1, 1), (1, 1), (1, 2))),
}


def yolo_switches():
    """The switches as the environment has them now."""
    return YoloSwitches(**{f: os.environ.get(name, "1") != "0" for f, (name, _, _) in SWITCH_TABLE.items()})


def yolo_lanes():
    """The lane mode the environment asks for now (default 3)."""
    return int(os.environ.get(LANES_VARIABLE, "3"))


# ---- the network ----------------------------------------------------------------------------------------------------------------------------
SCALES = {"n": (0.50, 0.25, 1024), "s": (0.50, 0.50, 1024), "m": (0.50, 1.00, 512),       # depth, width, max_channels
          "l": (1.00, 1.00, 512), "x": (1.00, 1.50, 512)}


def make_divisible(x, d=8):
    return int(math.ceil(x / d) * d)


def scale_fns(scale):
    """(ch, rep) of a scale letter: yolo11.yaml's channel count -> this scale's; its repeat count -> this scale's."""
    d, w, mc = SCALES[scale]
    return (lambda c: make_divisible(min(c, mc) * w, 8)), (lambda n: max(round(n * d), 1) if n > 1 else n)


class Layer(NamedTuple):
    name: str                     # ultralytics' module name, `model.N`
    op: str                       # "stem" | "conv" | "c3k2" | "sppf" | "c2psa" | "detect"
    srcs: tuple                   # ((layer name, upsample), ...): channel-concatenated, a source with upsample = 1 read 2x nearest-upsampled
    c1: object                    # input channels, summed over the sources (detect: the tuple of its levels' widths; stem: the image's 3)
    c2: int                       # output channels (detect: the class count)
    k: int = 1
    s: int = 1
    n: int = 1                    # inner blocks of a c3k2 / c2psa
    c3k: bool = False             # c3k2: the inner blocks are C3k(n = 2), not Bottleneck
    e: float = 0.5                # c3k2: hidden width c = int(c2 * e)


def yolo_layers(scale, nc):
    """YOLO11 (yolo11.yaml): one Layer per module that owns parameters or launches, model.0 .. model.23.  Upsample (11, 14) and Concat (12, 15, 18,
    21) are never materialised: they are the `srcs` of the layer that reads them."""
    ch, rep = scale_fns(scale)
    ca, n = scale in "mlx", rep(2)
    table = [
        ("model.0", "stem", (), ch(64), dict(k=3, s=2)),
        ("model.1", "conv", ("model.0",), ch(128), dict(k=3, s=2)),
        ("model.2", "c3k2", ("model.1",), ch(256), dict(n=n, c3k=ca, e=0.25)),
        ("model.3", "conv", ("model.2",), ch(256), dict(k=3, s=2)),
        ("model.4", "c3k2", ("model.3",), ch(512), dict(n=n, c3k=ca, e=0.25)),                # P3
        ("model.5", "conv", ("model.4",), ch(512), dict(k=3, s=2)),
        ("model.6", "c3k2", ("model.5",), ch(512), dict(n=n, c3k=True)),                      # P4
        ("model.7", "conv", ("model.6",), ch(1024), dict(k=3, s=2)),
        ("model.8", "c3k2", ("model.7",), ch(1024), dict(n=n, c3k=True)),
        ("model.9", "sppf", ("model.8",), ch(1024), dict(k=5)),
        ("model.10", "c2psa", ("model.9",), ch(1024), dict(n=n)),                             # P5
        ("model.13", "c3k2", (("model.10", 1), "model.6"), ch(512), dict(n=n, c3k=ca)),
        ("model.16", "c3k2", (("model.13", 1), "model.4"), ch(256), dict(n=n, c3k=ca)),       # Detect level 0
        ("model.17", "conv", ("model.16",), ch(256), dict(k=3, s=2)),
        ("model.19", "c3k2", ("model.17", "model.13"), ch(512), dict(n=n, c3k=ca)),           # Detect level 1
        ("model.20", "conv", ("model.19",), ch(512), dict(k=3, s=2)),
        ("model.22", "c3k2", ("model.20", "model.10"), ch(1024), dict(n=n, c3k=True)),        # Detect level 2
        ("model.23", "detect", ("model.16", "model.19", "model.22"), nc, {}),
    ]
    layers, width = [], {}
    for name, op, srcs, c2, kw in table:
        srcs = tuple(s if isinstance(s, tuple) else (s, 0) for s in srcs)
        cs = tuple(width[s] for s, _ in srcs)
        layers.append(Layer(name, op, srcs, 3 if op == "stem" else cs if op == "detect" else sum(cs), c2, **kw))
        width[name] = c2
    return layers


# ---- what each layer is made of ----------------------------------------------------------------------------------------------------------------
class ConvSpec(NamedTuple):
    """One packed convolution: `key` of Yolo11Weights.packed (and, but for "pair" / "dw_heads", the ultralytics module that owns the parameters)."""
    key: str
    c1: int
    c2: int
    k: int
    form: str = "conv"            # "conv" (Conv2d + BN) | "stem" (model.0 on the space-to-depth image) | "pair" (`...cv12`: cv1 and cv2 of a C3k,
                                  # c2 wide each, stacked along Cout) | "dw" (depthwise Conv2d + BN) | "dw_heads" (one depthwise conv packed per
                                  # attention head, `key.h{h}`) | "plain" (Conv2d with bias, no BN)


def bottleneck_convs(name, c, e):
    return [ConvSpec(f"{name}.cv1", c, int(c * e), 3), ConvSpec(f"{name}.cv2", int(c * e), c, 3)]


def c3k_convs(name, c):
    c_ = int(c * 0.5)
    return ([ConvSpec(f"{name}.cv12", c, c_, 1, "pair")] + [s for i in range(2) for s in bottleneck_convs(f"{name}.m.{i}", c_, 1.0)]
            + [ConvSpec(f"{name}.cv3", 2 * c_, c, 1)])


def c3k2_widths(L):
    """(c, h): a C3k2's hidden width and, where its inner blocks are Bottlenecks, theirs."""
    c = int(L.c2 * L.e)
    return c, int(c * 0.5)


def c3k2_convs(L):
    c, _ = c3k2_widths(L)
    inner = [s for i in range(L.n) for s in (c3k_convs(f"{L.name}.m.{i}", c) if L.c3k else bottleneck_convs(f"{L.name}.m.{i}", c, 0.5))]
    return [ConvSpec(f"{L.name}.cv1", L.c1, 2 * c, 1)] + inner + [ConvSpec(f"{L.name}.cv2", (2 + L.n) * c, L.c2, 1)]


class PsaGeometry(NamedTuple):
    cp: int                       # width of each half of cv1's output; the attention runs on the second
    heads: int
    kd: int                       # q / k width per head
    hd: int                       # v width per head: a head's rows of the qkv output are [q (kd) | k (kd) | v (hd)]
    per: int                      # 2 * kd + hd
    qkv: int                      # heads * per


PSA_KD, PSA_HD = 32, 64


def c2psa_geometry(L):
    cp, kd, hd = L.c2 // 2, PSA_KD, PSA_HD
    assert cp % hd == 0, L
    return PsaGeometry(cp, cp // hd, kd, hd, 2 * kd + hd, cp // hd * (2 * kd + hd))


def c2psa_convs(L):
    g, out = c2psa_geometry(L), [ConvSpec(f"{L.name}.cv1", L.c1, L.c2, 1), ConvSpec(f"{L.name}.cv2", L.c2, L.c2, 1)]
    for i in range(L.n):
        m = f"{L.name}.m.{i}"
        out += [ConvSpec(f"{m}.attn.qkv", g.cp, g.qkv, 1), ConvSpec(f"{m}.attn.proj", g.cp, g.cp, 1),
                ConvSpec(f"{m}.attn.pe", g.cp, g.cp, 3, "dw_heads"),       # the positional depthwise conv acts on v: one hd-channel slice per head
                ConvSpec(f"{m}.ffn.0", g.cp, 2 * g.cp, 1), ConvSpec(f"{m}.ffn.1", 2 * g.cp, g.cp, 1)]
    return out


class DetectGeometry(NamedTuple):
    ch: tuple                     # width of each level's feature map
    c2: int                       # box branch
    c3: int                       # class branch
    ncp: int                      # class count padded to 8: the channel count of a level's class buffer


def detect_geometry(L):
    return DetectGeometry(L.c1, max(16, L.c1[0] // 4, 64), max(L.c1[0], min(L.c2, 100)), (L.c2 + 7) // 8 * 8)


def detect_convs(L, i):
    """Level i: [box branch, class branch]."""
    g, x = detect_geometry(L), L.c1[i]
    b, c = f"{L.name}.cv2.{i}", f"{L.name}.cv3.{i}"
    return ([ConvSpec(f"{b}.0", x, g.c2, 3), ConvSpec(f"{b}.1", g.c2, g.c2, 3), ConvSpec(f"{b}.2", g.c2, 64, 1, "plain")],
            [ConvSpec(f"{c}.0.0", x, x, 3, "dw"), ConvSpec(f"{c}.0.1", x, g.c3, 1), ConvSpec(f"{c}.1.0", g.c3, g.c3, 3, "dw"),
             ConvSpec(f"{c}.1.1", g.c3, g.c3, 1), ConvSpec(f"{c}.2", g.c3, L.c2, 1, "plain")])


def layer_convs(L):
    """Every ConvSpec of a layer, in the order Yolo11Weights pulls and packs them."""
    if L.op in ("stem", "conv"):
        return [ConvSpec(L.name, L.c1, L.c2, L.k, L.op)]
    if L.op == "sppf":
        return [ConvSpec(f"{L.name}.cv1", L.c1, L.c1 // 2, 1), ConvSpec(f"{L.name}.cv2", 2 * L.c1, L.c2, 1)]
    if L.op == "detect":
        return [s for i in range(len(L.c1)) for branch in detect_convs(L, i) for s in branch]
    return dict(c3k2=c3k2_convs, c2psa=c2psa_convs)[L.op](L)


# ---- the route --------------------------------------------------------------------------------------------------------------------------------
class YoloRoute(NamedTuple):
    layers: tuple                 # yolo_layers
    stem: str                     # "fused" (model.0 + model.1 in one launch, label `model.0-1`) | "chain"
    c3k2: dict                    # per C3k2 layer: "fused_cv1" (one launch, label `model.N`) | "fused" (`model.N.cv1`, `model.N.fused`) | "chain"
    cls: tuple                    # per Detect level, the class branch: "dwpw" (two launches, `...cv3.i.0` and `...cv3.i.1-2`) | "chain" (five)
    lanes: Optional[tuple]        # per Detect level (box lane, class lane) of the captured graph; None: no fork, everything on lane 0

    def launches(self, with_nms=True):
        """[(label, kind, lane)] in launch order, the `fork` / `join` sync entries with their -1 / -2 lane marks.  A second statement of the order
        in which `Yolo11Plan` emits, kept for the tests: the fixture test derives sequences from it without a GPU, and tests/test_yolo_route_gpu.py
        holds the emitter to it -- change the two together."""
        conv = lambda *labels: [(l, "conv", 0) for l in labels]
        det = self.layers[-1]
        level_of = {s: i for i, (s, _) in enumerate(det.srcs)}
        out = []
        for L in self.layers[:-1]:
            if L.op == "stem":
                out += [("model.0-1", "stem", 0)] if self.stem == "fused" else [(L.name, "stem", 0)]
            elif L.op == "conv":
                out += [] if L.srcs[0][0] == "model.0" and self.stem == "fused" else conv(L.name)
            elif L.op == "c3k2":
                mode = self.c3k2[L.name]
                out += conv(L.name) if mode == "fused_cv1" else conv(f"{L.name}.cv1", f"{L.name}.fused") if mode == "fused" else conv(*(s.key for s in c3k2_convs(L)))
            elif L.op == "sppf":
                out += conv(f"{L.name}.cv1") + [(f"{L.name}.pool", "pool", 0)] + conv(f"{L.name}.cv2")
            elif L.op == "c2psa":
                out += conv(f"{L.name}.cv1")
                for i in range(L.n):
                    m = f"{L.name}.m.{i}"
                    out += conv(f"{m}.attn.qkv") + [(f"{m}.attn.sdpa", "attention", 0)]
                    out += [(f"{m}.attn.pe.h{h}", "dwconv", 0) for h in range(c2psa_geometry(L).heads)] + conv(f"{m}.attn.proj", f"{m}.ffn.0", f"{m}.ffn.1")
                out += conv(f"{L.name}.cv2")
            if L.name in level_of:
                i = level_of[L.name]
                box_lane, cls_lane = self.lanes[i] if self.lanes else (0, 0)
                box, cls = detect_convs(det, i)
                out += [("fork", "sync", -1)] if self.lanes else []
                out += [(s.key, "head", box_lane) for s in box]
                if self.cls[i] == "dwpw":
                    out += [(f"{det.name}.cv3.{i}.0", "head", cls_lane), (f"{det.name}.cv3.{i}.1-2", "head", cls_lane)]
                else:
                    out += [(s.key, "dwconv" if s.form == "dw" else "head", cls_lane) for s in cls]
        return out + [("join", "sync", -2), (f"{det.name}.decode", "decode", 0)] + ([("nms", "nms", 0)] if with_nms else [])


def route_yolo(scale, nc, dtype, sw: YoloSwitches, lanes):
    """Route of a detector plan.  sw: the plan's switches; lanes: a LANE_MODES mode."""
    if lanes not in LANE_MODES:
        raise ValueError(f"lane mode {lanes!r}: {LANES_VARIABLE} / Yolo11Plan(lanes=) takes one of {sorted(LANE_MODES)}")
    layers = tuple(yolo_layers(scale, nc))
    c3k2 = {}
    for L in layers:
        if L.op == "c3k2":
            c, h = c3k2_widths(L)
            one_src = len(L.srcs) == 1 and L.srcs[0][1] == 0
            # small-channel blocks: one fused launch (c3k2_fused.hip), with cv1 folded in when the block has a single source
            small = sw.fuse_c3k2 and not L.c3k and L.n == 1
            c3k2[L.name] = ("fused_cv1" if small and one_src and c3k2_supported(L.c1, c, h, L.c2, True, dtype)
                            else "fused" if small and c3k2_supported(0, c, h, L.c2, False, dtype) else "chain")
    g = detect_geometry(layers[-1])
    return YoloRoute(
        layers=layers, stem="fused" if sw.fuse_stem and stem2_supported(layers[0].c2, layers[1].c2, dtype) else "chain", c3k2=c3k2,
        # class branch in two launches: [dw3x3 + 1x1], [dw3x3 + 1x1 + class 1x1]; the intermediates stay in LDS -- when both configurations are built
        cls=tuple("dwpw" if sw.fuse_dwpw and dwpw_supported(x, g.c3, 0, dtype) and dwpw_supported(g.c3, g.c3, nc, dtype) else "chain" for x in g.ch),
        lanes=LANE_MODES[lanes][1])
