#!/usr/bin/env python3
"""A/B of two builds of libcvmi355.so on cvmi_conv2d, one build per process (CVMI_LIB_PATH selects it): profiles/conv_epilogue_refactor_ab.md.

  hash  every CONV_ROWS row (tests/op_matrix.py) in every dtype it allows, the "random" operand structure of tests/test_conv_matrix_gpu.py with
        its fixed seeds: one line "row dtype tag sha256(whole output buffer, padding columns and the spare image included) sha256(row_stats)".
        Two builds compute the same thing iff their outputs of this mode are equal as text.
  time  event-timed launches at shapes of bench.py's workloads (YOLO11-n / -l at 640 x 640, SAM 2.1 Hiera-L at 1024 x 1024): per shape the tag
        and the median in microseconds of --launches launches after 5 warm-up launches.
"""
import argparse
import hashlib
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

from circuitvision_amd import _lib  # noqa: E402
from circuitvision_amd._lib import ACT_GELU, ACT_NONE, ACT_SILU, F16, F32  # noqa: E402
from circuitvision_amd.engine import TORCH_DTYPE, Buf, PackedConv, Plan, op_conv  # noqa: E402

# (id, B, Cin, H, W, Cout, k, stride, act, residual, f32 output): 16-bit operands
TIME_SHAPES = [
    ("n_3x3s2_16_32_320", 32, 16, 320, 320, 32, 3, 2, ACT_SILU, False, False),         # YOLO11-n model.1
    ("n_3x3s1_32_32_160_res", 32, 32, 160, 160, 32, 3, 1, ACT_SILU, True, False),      # YOLO11-n bottleneck with shortcut
    ("n_3x3s2_64_128_80", 32, 64, 80, 80, 128, 3, 2, ACT_SILU, False, False),          # YOLO11-n model.5
    ("n_1x1_64_128_160", 32, 64, 160, 160, 128, 1, 1, ACT_SILU, False, False),         # YOLO11-n C3k2 cv2 at the 160 x 160 level
    ("n_1x1_128_128_80", 32, 128, 80, 80, 128, 1, 1, ACT_SILU, False, False),          # YOLO11-n C3k2 cv2 at the 80 x 80 level
    ("n_1x1_256_256_20_res", 32, 256, 20, 20, 256, 1, 1, ACT_NONE, True, False),       # YOLO11-n C2PSA projection + shortcut
    ("n_3x3s1_256_64_20", 32, 256, 20, 20, 64, 3, 1, ACT_SILU, False, False),          # YOLO11-n Detect cv2.2.0 (split-K)
    ("l_3x3s1_128_128_160_res", 8, 128, 160, 160, 128, 3, 1, ACT_SILU, True, False),   # YOLO11-l bottleneck with shortcut
    ("l_3x3s1_256_256_80", 8, 256, 80, 80, 256, 3, 1, ACT_SILU, False, False),         # YOLO11-l bottleneck on the 256-tile pipeline
    ("h_s4_proj_1152_f32res", 16, 1152, 32, 32, 1152, 1, 1, ACT_NONE, True, True),     # Hiera-L stage-4 proj
    ("h_s4_fc2_4608_f32res", 16, 4608, 32, 32, 1152, 1, 1, ACT_NONE, True, True),      # Hiera-L stage-4 fc2
    ("h_s4_qkv_3456_res16", 16, 1152, 32, 32, 3456, 1, 1, ACT_NONE, True, False),      # stage-4 qkv shape, 16-bit out + residual: gemm256_kernel<f16>
    ("h_s3_qkv_1728_f32res", 16, 576, 64, 64, 1728, 1, 1, ACT_NONE, True, True),       # stage-3 qkv shape, f32 out + residual: gemm256_kernel<float>, two passes
    ("h_s3_fc2_gelu_f32res", 16, 2304, 64, 64, 576, 1, 1, ACT_GELU, True, True),       # stage-3 fc2 shape with an activation: gemm256x192_kernel<float>'s LDS epilogue
    ("h_s3_fc2_res16", 16, 2304, 64, 64, 576, 1, 1, ACT_NONE, True, False),            # the same, 16-bit out: gemm256x192_kernel<f16>
    ("h_s3_proj_576_f32res", 16, 576, 64, 64, 576, 1, 1, ACT_NONE, True, True),        # stage-3 proj: gemm_glds_kernel (gemm_epilogue, prefetched residual)
]


def mode_hash():
    import test_conv_matrix_gpu as T
    from op_matrix import CONV_ROWS
    lib = _lib.load()
    ncu = T._cu_count(lib)
    made = []

    class RecBuf(Buf):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)

    T.Buf = RecBuf
    for row in CONV_ROWS:
        if row["B"] == "cu/2" and ncu % 8 != 0:
            continue
        for dt in row["dtypes"]:
            dtype = T.DT[dt]
            odt = F32 if (dtype == F32 or row["out_f32"]) else dtype
            geo = T._geometry(row, ncu)
            g = torch.Generator().manual_seed(1000 + 7 * geo[7] + row["Cout"] + geo[0])
            srcs, w, b, r = T._operands("random", row, dtype, odt, geo, g)
            del made[:]
            tag, _, same, _, stats = T._launch(row, dtype, odt, geo, srcs, w, b, r, T.ACT[row["act"]], lib)
            y = made[len(srcs)].t                                         # the whole output buffer (Buf order in _launch: sources, output, residual)
            hy = hashlib.sha256(y.cpu().view(torch.uint8).numpy().tobytes()).hexdigest()
            hs = hashlib.sha256(stats.numpy().tobytes()).hexdigest() if stats is not None else "-"
            print(f"{row['id']} {dt} {tag} {hy} {hs} {'rerun-equal' if same else 'RERUN-DIFFERS'}", flush=True)


def mode_time(launches):
    lib = _lib.load()
    g = torch.Generator(device="cuda").manual_seed(5)
    for rid, B, Cin, H, W, N, k, s, act, res, f32out in TIME_SHAPES:
        OH, OW = (H + 2 * (k // 2) - k) // s + 1, (W + 2 * (k // 2) - k) // s + 1
        odt = F32 if f32out else F16
        xb, yb = Buf(B, H, W, Cin, F16), Buf(B, OH, OW, N, odt)
        xb.t.copy_(torch.randn(xb.t.shape, generator=g, device="cuda").to(torch.float16))
        rb = None
        if res:
            rb = Buf(B, OH, OW, N, odt)
            rb.t.copy_(torch.randn(rb.t.shape, generator=g, device="cuda").to(TORCH_DTYPE[odt]))
        pc = PackedConv(torch.randn(N, Cin, k, k) / (Cin * k * k) ** 0.5, torch.randn(N), F16)
        plan = Plan(torch.cuda.Stream())
        op_conv(plan, rid, pc, [(xb.view(), 0)], yb.view(), stride=s, act=act, res=rb.view() if rb else None)
        torch.cuda.synchronize()
        lib.cvmi_last_kernel()
        times = []
        with torch.cuda.stream(plan.stream):
            for i in range(5 + launches):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(plan.stream)
                plan.run_eager()
                e1.record(plan.stream)
                e1.synchronize()
                if i >= 5:
                    times.append(e0.elapsed_time(e1) * 1e3)
        print(f"{rid} | {lib.cvmi_last_kernel().decode()} | {statistics.median(times):.2f}", flush=True)
        del plan, xb, yb, rb, pc
        torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("hash", "time"))
    ap.add_argument("--launches", type=int, default=30)
    a = ap.parse_args()
    mode_hash() if a.mode == "hash" else mode_time(a.launches)
