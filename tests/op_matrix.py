"""Case tables shared by the per-op GPU suites and the CPU coverage guard (tests/test_op_coverage_cpu.py).

ATTN_ROWS / ATTN_FP8_ROWS / ATTN_FP8_FALLBACK_ROWS: the attention dispatch matrix.  One row = one shape and layout of cvmi_attention and the kernel that cvmi_last_kernel() must name
after the launch (attention.hip, cvmi_attention: the dispatcher with default settings).  Kernel names do not carry the operand type, so one
expected name serves fp16 and bf16.

CONV_ROWS: the convolution / GEMM dispatch matrix.  One row = one cvmi_conv2d descriptor (shape + epilogue options) and the kernel tag
cvmi_last_kernel() must name (igemm.hip launch_typed / launch_cfg / launch_glds / launch_g256*, conv_tile.hip launch_tile_*).  Tags carry the
operand type, and the bf16 build has no conv_tile path, so `expect` is a string with a {T} placeholder (the operand type as the tag spells it)
or a dict per dtype of such strings.

FUSED_ROWS: the fused YOLO11 kernels.  One row = one launch of cvmi_c3k2, cvmi_stem2 or cvmi_dwpw, the tag it must report (launch_c3k2 / launch_dwpw /
cvmi_stem2 tag the instance as the template is written) and its options; operands, references and the tolerance live in tests/fused_ref.py.

LN_ROWS / LN_DUAL_ROWS: cvmi_layernorm and cvmi_layernorm_dual.  One row = one launch, the template instance layernorm_kernel<TI, TO, NCH, WD>
that launch_ln (sam_ops.hip) must tag, and the lanes per row G that ln_pick -- a mirror of launch_ln's selection loop -- derives from C.  The
rows are generated from ln_pick: every reachable (G, NCH) of every form at the smallest C that selects it, plus the row counts, layouts and
options at which a row-per-lane-group kernel goes wrong.

HELPER_ROWS: the other helper kernels of sam_ops.hip and vision_ops.hip (SPPF pooling, the refinement head, depthwise 3x3, the grid-capped
copies, bilinear resize / mask post-processing, the mask decoder tail).  Operands, references and tolerances live in tests/helper_ref.py.

TOK_ROWS / MLP_ROWS: the token-stationary path (tok_linear.hip, tok_linear16.hip, hiera_mlp.hip).  One row = one launch through engine.py's wrappers and
the template instance its dispatcher must tag; tok_pick / tl16_splits / mlp_pick mirror tok_dispatch, launch_tl's staged-store rule, the POOL call
sites, the K = 576 hand-over and its row-block sharing, and generate TOK_INSTANCES / MLP_INSTANCES.  Operands, references and tolerances live in
tests/tok_ref.py.  tl16_splits is compared with the library's own answer (cvmi_tok_linear_stats_parts) on the GPU for every N % 32 == 0 of the table;
its N % 32 != 0 branch is checked by reading only: the library exports the split count through that entry point alone, which always asks for the
statistics-out form, where a ragged N never splits; the split count is not in the tag.

PROJ_ROWS / MLP_KIND_ROWS: the proj + MLP launch (proj_mlp.hpp) at every row count of MLP_ROW_COUNTS, and one launch per proj_mlp / hiera_mlp
instance whose LayerNorm input carries the five row kinds (KIND_BLOCKS); proj_pick mirrors proj_mlp_dispatch.

NMS_ROWS / DECODE_ROWS: the detector's tail (nms.hip, vision_ops.hip cvmi_detect_decode).  One NMS row = one input with an exact candidate count, the
instance nms_launch must tag and the decisions nms_pick -- a mirror of nms_launch and of yolo_nms_kernel's data-dependent branches -- derives from it; one
decode row = one launch per dtype with its stated seams.  Generators, references, mutants and the decode bound live in tests/detect_ref.py.

RESAMPLE_ROWS: the resampling kernels of resample.hip (the five forms of cvmi_sam2_transform*, the four forms of the bilinear mask return and
cvmi_mask_extent).  One row = the sources, windows or sizes of one call and the entry forms, output types and swap_rb values it runs through; the
constants the rows were built from (AA_MAXTAPS, RECT_MAX, the grid caps) mirror the source text.  Operands, references, mutants and bounds live in
tests/resample_ref.py.

CONTOUR_ROWS / PREPARE_ROWS: the contour stage of wire_ops.hip (cvmi_external_contours' ten kernels, cvmi_node_prepare).  One contour row = one batch
of plane specs and the trace tag (path and dynamic LDS bytes) the call must report; contour_tag mirrors the per-batch choice, and the constants
the shapes were sized from (PLANE_MAX, the launch shapes, the two LDS thresholds) mirror the source text.  Plane builders, the geometric oracle
and the float64 resize live in tests/contour_ref.py.

BF16_OPS: every entry point that common.hpp builds twice (CVMI_ENTRY) -> (test module, test function) that checks its bf16 build per op.

Plain data: importing this module needs neither a GPU nor the library."""

F16_BF16 = ("f16", "bf16")


def _row(rid, expect, B, heads, Nq, Nk, dqk, dv, dtypes=F16_BF16, layout="sep", o_pad=0, q_log2=0, av_fp8=0, note=""):
    """Global (non-window) attention.  layout: "sep" = q, k, v in three [B, N, heads * d] buffers; "qkv" = one fused [B, N, (2 dqk + dv) heads]
    buffer (needs Nq == Nk); "kv256" = the decoder's K and V halves of one [B, Nk, heads * (dqk + dv)] buffer.  o_pad > 0: the output sits at
    column o_pad of a buffer o_pad columns wider on both sides.  av_fp8: cvmi_attn_desc.av_fp8 as the launch sets it."""
    return dict(id=rid, expect=expect, B=B, heads=heads, Nq=Nq, Nk=Nk, dqk=dqk, dv=dv, dtypes=dtypes, layout=layout, o_pad=o_pad,
                q_log2=q_log2, av_fp8=av_fp8, win=0, note=note)


def _win(rid, expect, imgs, gh, gw, heads, win, q_pool=0, dtypes=F16_BF16, o_pad=0, q_log2=0, av_fp8=0, note=""):
    """Hiera window attention straight off a fused NHWC [imgs, gh, gw, 3 C] q/k/v grid (k_st = 3 C), head_dim 72, optional 2 x 2 q max-pool."""
    nwin = imgs * (gh // win) * (gw // win)
    Nq = (win // 2) ** 2 if q_pool else win * win
    return dict(id=rid, expect=expect, B=nwin, heads=heads, Nq=Nq, Nk=win * win, dqk=72, dv=72, dtypes=dtypes, layout="grid", o_pad=o_pad,
                q_log2=q_log2, av_fp8=av_fp8, win=win, imgs=imgs, gh=gh, gw=gw, q_pool=q_pool, note=note)


ATTN_ROWS = [
    # ---- 4 x 4 windows: the per-thread VALU kernel (8 items per workgroup: 36 and 18 items leave idle lanes in the last one)
    _win("win4", "attn_win16_kernel<16, 9>", 2, 8, 12, 3, 4, o_pad=8),
    _win("win4_pool", "attn_win16_kernel<4, 9>", 1, 8, 12, 3, 4, q_pool=1),
    # ---- 256 keys
    _win("win16", "attn_res256_kernel<8, false, false>", 2, 16, 32, 2, 16),
    _win("win16_pool", "attn_res256_kernel<4, false, false>", 2, 16, 32, 2, 16, q_pool=1, o_pad=8),
    _row("g256", "attn_res256_kernel<8, false, false>", 2, 2, 256, 256, 72, 72, layout="qkv"),
    _row("g256_nq225", "attn_res256_kernel<8, false, false>", 1, 3, 225, 256, 72, 72, note="Nq = 1 mod 32: one valid row in the last q tile"),
    _row("g256_nq223", "attn_res256_kernel<4, false, false>", 1, 3, 223, 256, 72, 72, o_pad=8, note="Nq = 31 mod 32"),
    _row("g256_nq161", "attn_res256_kernel<4, false, false>", 2, 1, 161, 256, 72, 72),
    # ---- 256 keys, q pre-scaled by scale * log2(e)
    _win("win16_qlog2", "attn_res256_kernel<8, false, true>", 2, 16, 32, 2, 16, q_log2=1),
    _win("win16_pool_qlog2", "attn_res256_kernel<4, false, true>", 2, 16, 32, 2, 16, q_pool=1, q_log2=1),
    _row("g256_nq200_qlog2", "attn_res256_kernel<4, false, true>", 1, 2, 200, 256, 72, 72, q_log2=1),
    # ---- 64 keys
    _win("win8", "attn_res64_kernel<2>", 2, 16, 24, 2, 8),
    _win("win8_pool", "attn_res64_kernel<1>", 2, 16, 24, 2, 8, q_pool=1, o_pad=8),
    _row("g64", "attn_res64_kernel<2>", 3, 2, 64, 64, 72, 72, layout="qkv"),
    _row("g64_nq33", "attn_res64_kernel<2>", 2, 2, 33, 64, 72, 72),
    _row("g64_nq31", "attn_res64_kernel<1>", 2, 2, 31, 64, 72, 72),
    # ---- long sequences in whole 64-key tiles (19 / 17 q tiles: idle waves in the last workgroup)
    _row("dma72_600x640", "attn_dma72_kernel<8, false, false>", 2, 3, 600, 640, 72, 72),
    _row("dma72_1024", "attn_dma72_kernel<8, false, false>", 1, 2, 1024, 1024, 72, 72, layout="qkv"),
    _row("dma72_nq577", "attn_dma72_kernel<8, false, false>", 1, 2, 577, 576, 72, 72, o_pad=8),
    _row("dma72_nq543", "attn_dma72_kernel<8, false, false>", 1, 2, 543, 512, 72, 72),
    _row("dma72_qlog2", "attn_dma72_kernel<8, false, true>", 1, 2, 600, 640, 72, 72, q_log2=1),
    # ---- general kernel, >= 8 query tiles per (batch, head)
    _row("i2t", "attn64_kernel<32, 32, 8>", 1, 8, 4096, 8, 16, 16, note="mask decoder image -> token"),
    _row("i2t_nk1", "attn64_kernel<32, 32, 8>", 1, 8, 4096, 1, 16, 16),
    _row("i2t_nk7", "attn64_kernel<32, 32, 8>", 1, 8, 4096, 7, 16, 16, o_pad=8),
    _row("c2psa", "attn64_kernel<32, 64, 8>", 2, 2, 400, 400, 32, 64, layout="qkv", o_pad=8),
    _row("g600", "attn64_kernel<96, 96, 8>", 2, 3, 600, 600, 72, 72),
    _row("g289", "attn64_kernel<96, 96, 8>", 1, 2, 289, 289, 72, 72, layout="qkv", note="Nq = Nk = 1 mod 32"),
    _row("g287x255", "attn64_kernel<96, 96, 8>", 1, 2, 287, 255, 72, 72, note="Nq = Nk = 31 mod 32"),
    _row("d64_8", "attn64_kernel<64, 64, 8>", 1, 2, 300, 200, 64, 64),
    _row("d128_8", "attn64_kernel<128, 128, 8>", 1, 1, 260, 100, 128, 128, o_pad=8),
    # ---- general kernel, 4-7 query tiles
    _row("g130x257", "attn64_kernel<96, 96, 4>", 1, 2, 130, 257, 72, 72, note="Nk = 1 mod 32"),
    _row("d64_4", "attn64_kernel<64, 64, 4>", 1, 2, 200, 333, 64, 64),
    _row("d64_4_nk31", "attn64_kernel<64, 64, 4>", 1, 2, 97, 31, 64, 64, note="Nq = 1 mod 32, Nk < 32"),
    _row("d128_4", "attn64_kernel<128, 128, 4>", 1, 2, 100, 130, 128, 128),
    _row("d32_4", "attn64_kernel<32, 32, 4>", 2, 2, 127, 225, 32, 32, note="Nq = 31, Nk = 1 mod 32"),
    # ---- 2-3 query tiles against >= 2048 keys: learned-prompt token -> image attention
    _row("t2i_learned", "attn64_kernel<32, 32, 4>", 1, 8, 38, 4096, 16, 16, layout="kv256"),
    _row("t2i_nq33", "attn64_kernel<32, 32, 4>", 1, 8, 33, 2049, 16, 16, note="Nq, Nk = 1 mod 32"),
    _row("t2i_nq95", "attn64_kernel<32, 32, 4>", 1, 8, 95, 2079, 16, 16, layout="kv256", o_pad=8, note="Nq, Nk = 31 mod 32"),
    # ---- one query tile per wave
    _row("t2i_boxes", "attn_f16_kernel<32, 32, 64>", 1, 8, 8, 4096, 16, 16, layout="kv256"),
    _row("t2i_nk2049", "attn_f16_kernel<32, 32, 64>", 1, 8, 8, 2049, 16, 16),
    _row("tok_self", "attn_f16_kernel<32, 32, 64>", 1, 8, 8, 8, 32, 32, layout="qkv"),
    _row("nq1_nk1", "attn_f16_kernel<32, 32, 64>", 1, 8, 1, 1, 32, 32),
    _row("nq31_nk7", "attn_f16_kernel<32, 32, 64>", 1, 8, 31, 7, 16, 16, o_pad=8),
    _row("nq33_nk33", "attn_f16_kernel<32, 32, 64>", 3, 1, 33, 33, 16, 16),
    _row("d32x64_1", "attn_f16_kernel<32, 64, 64>", 2, 2, 20, 50, 32, 64),
    _row("d64_1", "attn_f16_kernel<64, 64, 64>", 2, 2, 50, 31, 64, 64),
    _row("tiny_win", "attn_f16_kernel<96, 96, 64>", 5, 3, 16, 16, 72, 72, note="15 items: idle waves in the last workgroup"),
    _row("d128_1", "attn_f16_kernel<128, 128, 64>", 1, 1, 40, 70, 128, 128),
    # ---- fp32 parity mode
    _row("f32_general", "attn_f32_kernel", 2, 2, 130, 257, 72, 72, dtypes=("f32",), o_pad=8),
    _win("f32_win8", "attn_f32_kernel", 2, 16, 24, 2, 8, dtypes=("f32",)),
]

# The e4m3 AV-product instances (cvmi_attn_desc.av_fp8 = 1): attn_res256_kernel<8, true, false> and attn_dma72_kernel<8, true, false>, f16 and
# bf16, head dim 72, at the smallest shape at which each edge of their index arithmetic exists.  q_log2 = 1 beside av_fp8 = 1 is what
# sam2.py:_attn_desc sets in production: the dispatcher gives fp8 precedence, the tag stays <8, true, false> and the kernel runs with scale = ln 2.
# Operands, the float64 emulation, its derived bound and the mutants live in tests/attn_fp8_ref.py.
RES256_FP8, DMA72_FP8 = "attn_res256_kernel<8, true, false>", "attn_dma72_kernel<8, true, false>"
ATTN_FP8_ROWS = [
    # ---- 256 keys, >= 8 query tiles: all 8 waves build the e4m3 V image, whether their query tile is live or not
    _win("win16_fp8", RES256_FP8, 2, 16, 32, 2, 16, av_fp8=1),
    _win("win16_fp8_opad", RES256_FP8, 2, 16, 32, 2, 16, o_pad=8, av_fp8=1),
    _row("g256_fp8", RES256_FP8, 2, 2, 256, 256, 72, 72, layout="qkv", av_fp8=1),
    _row("g256_nq225_fp8", RES256_FP8, 1, 3, 225, 256, 72, 72, av_fp8=1, note="one valid row in the 8th q tile"),
    _row("g256_nq257_fp8", RES256_FP8, 1, 3, 257, 256, 72, 72, av_fp8=1, note="9 q tiles: a second query group, one live wave holding one valid row"),
    _row("g256_nq512_fp8", RES256_FP8, 1, 1, 512, 256, 72, 72, av_fp8=1, note="two full query groups on a single item: grid of 2"),
    _win("win16_fp8_qlog2", RES256_FP8, 2, 16, 32, 2, 16, q_log2=1, av_fp8=1),
    _row("g256_nq257_fp8_qlog2", RES256_FP8, 1, 3, 257, 256, 72, 72, q_log2=1, av_fp8=1),
    # ---- >= 512 keys in whole 64-key tiles
    _row("dma72_fp8_256x512", DMA72_FP8, 1, 2, 256, 512, 72, 72, av_fp8=1, note="fewest keys, fewest q tiles"),
    _row("dma72_fp8_nq543", DMA72_FP8, 1, 2, 543, 512, 72, 72, av_fp8=1, note="ragged last q tile"),
    _row("dma72_fp8_nq577", DMA72_FP8, 1, 2, 577, 576, 72, 72, o_pad=8, av_fp8=1, note="9 key tiles (odd): the last tile sits in buffer 0"),
    _row("dma72_fp8_600x640", DMA72_FP8, 2, 3, 600, 640, 72, 72, av_fp8=1, note="Nq != Nk, 6 items"),
    _row("dma72_fp8_1024", DMA72_FP8, 1, 2, 1024, 1024, 72, 72, layout="qkv", av_fp8=1),
    _row("dma72_fp8_600x640_qlog2", DMA72_FP8, 2, 3, 600, 640, 72, 72, q_log2=1, av_fp8=1),
    _row("dma72_fp8_1024_qlog2", DMA72_FP8, 1, 2, 1024, 1024, 72, 72, layout="qkv", q_log2=1, av_fp8=1),
]
# av_fp8 = 1 where the dispatcher drops it: the tag is the 16-bit instance, the result holds the 16-bit bound of the matrix and is bit-identical
# to the same launch with av_fp8 = 0.
ATTN_FP8_FALLBACK_ROWS = [
    _win("win16_pool_fp8", "attn_res256_kernel<4, false, false>", 2, 16, 32, 2, 16, q_pool=1, o_pad=8, av_fp8=1, note="2 q tiles"),
    _win("win16_pool_fp8_qlog2", "attn_res256_kernel<4, false, true>", 2, 16, 32, 2, 16, q_pool=1, q_log2=1, av_fp8=1),
    _row("g256_nq223_fp8", "attn_res256_kernel<4, false, false>", 1, 3, 223, 256, 72, 72, o_pad=8, av_fp8=1, note="7 q tiles"),
    _win("win8_fp8", "attn_res64_kernel<2>", 2, 16, 24, 2, 8, av_fp8=1),
    _row("g600_fp8", "attn64_kernel<96, 96, 8>", 2, 3, 600, 600, 72, 72, av_fp8=1, note="Nk % 64 != 0"),
    _win("win4_fp8", "attn_win16_kernel<16, 9>", 2, 8, 12, 3, 4, o_pad=8, av_fp8=1),
]

# mutant of tests/attn_fp8_ref.py -> (row id, operand kind, dtype) cases of which at least one must put it outside the derived bound
# (tests/test_attn_fp8_ref_cpu.py)
FP8_MUTANT_CASES = {
    "l_of_quantised_p": [("g256_nq225_fp8", "random", "f16"), ("dma72_fp8_256x512", "random", "f16")],
    "p_scale_2^7": [("g256_nq225_fp8", "exact", "f16"), ("dma72_fp8_256x512", "exact", "f16")],
    "p_truncated": [("g256_nq225_fp8", "random", "f16"), ("dma72_fp8_256x512", "random", "bf16")],
    "v_unclamped_saturates": [("g256_nq225_fp8", "random", "f16"), ("dma72_fp8_256x512", "random", "bf16")],
    "key_halves_swapped": [("g256_nq225_fp8", "random", "bf16"), ("dma72_fp8_256x512", "exact", "f16")],
    "d_tiles_swapped": [("g256_nq225_fp8", "exact", "bf16"), ("dma72_fp8_256x512", "random", "f16")],
    "tile_32": [("g256_nq225_fp8", "random", "f16"), ("dma72_fp8_256x512", "random", "f16")],
}

# Batch sharing (cvmi_attn_desc.q_bdiv / kv_bdiv) at the mask decoder's layer-0 shapes: B = images x NP (image, prompt) pairs.
# (mode, images, NP, heads, Nq, Nk, d, expected kernel)
SHARE_ROWS = [
    ("t2i", 2, 1, 8, 8, 4096, 16, "attn_f16_kernel<32, 32, 64>"),
    ("t2i", 2, 5, 8, 8, 4096, 16, "attn_f16_kernel<32, 32, 64>"),
    ("t2i", 1, 32, 8, 8, 4096, 16, "attn_f16_kernel<32, 32, 64>"),
    ("i2t", 2, 1, 8, 4096, 8, 16, "attn64_kernel<32, 32, 8>"),
    ("i2t", 2, 5, 8, 4096, 8, 16, "attn64_kernel<32, 32, 8>"),
    ("i2t", 1, 32, 8, 4096, 8, 16, "attn64_kernel<32, 32, 8>"),
]

ALL3 = ("f16", "bf16", "f32")
F16_F32 = ("f16", "f32")
TNAME = {"f16": "_Float16", "bf16": "__bf16", "f32": "float"}          # CVMI_F16NAME / "float" as igemm.hip and conv_tile.hip print them

# (BM, BN, WM, WN) of igemm_kernel as launch_typed passes them to launch_cfg
T256x32, T128x32, T128x64, T64x64, T128x128, T64x128 = (256, 32, 4, 1), (128, 32, 4, 1), (128, 64, 2, 2), (64, 64, 2, 2), (128, 128, 2, 2), (64, 128, 2, 2)


def ig(tile, bkb, plain, ks=1, to="{T}"):
    """igemm_kernel<T, TO, BM, BN, WM, WN, BKB, PLAIN, KS>"""
    return "igemm_kernel<{T}, %s, %d, %d, %d, %d, %d, %s, %d>" % ((to,) + tile + (bkb, "true" if plain else "false", ks))


def glds(bn, to="{T}"):
    return "gemm_glds_kernel<{T}, %s, 128, %d, 2, 2>" % (to, bn)


def tile(ks, s, cc, bn, th=8):
    """conv_tile_kernel<T, KS, S, CC, BN, WM, WN, TH>: the four tile forms are 32/8 (4 x 1 waves), 64/4, 64/8 and 128/8 (2 x 2 waves)"""
    return "conv_tile_kernel<{T}, %d, %d, %d, %d, %d, %d, %d>" % (ks, s, cc, bn, 4 if bn == 32 else 2, 1 if bn == 32 else 2, th)


G256, G256_F32 = "gemm256_kernel<{T}, true>", "gemm256_kernel<float, true>"
G256_I2C, G256_I2C_F32 = "gemm256_kernel<{T}, true, true>", "gemm256_kernel<float, true, true>"
G256P, G192, G192_F32, G192R = "gemm256p_kernel", "gemm256x192_kernel<{T}>", "gemm256x192_kernel<float>", "gemm256x192r_kernel"


def _conv(rid, expect, B, Cin, H, W, Cout, k=1, stride=1, dtypes=F16_BF16, pad=None, out_hw=None, act="none", res="none", res_rep=0,
          act_after_res=False, shuffle_cout=0, out_f32=False, y_pad=0, scalar_gather=False, up=None, row_stats=False, note=""):
    """One cvmi_conv2d launch on an NHWC [B, H, W, Cin] input (H, W: the logical size, after upsampling).  Cin: an int, or (c0, c1) for two
    channel-concatenated sources of which source `up` (0 / 1 / None) is stored at half resolution.  B = "cu/2": half the device's CU count
    (gemm256x192r_kernel needs whole rounds of tiles).  pad None = k // 2.  res: "none" | "full" (one value per output element) | "bcast"
    (one [OH * OW, Cout] table for every image: res_mod) | "rep" (B / res_rep residual images, image b reads b / res_rep).  out_f32: f32
    output and residual from 16-bit operands.  y_pad > 0: the output (and a full residual) sit at channel y_pad of a buffer y_pad channels
    wider on both sides.  act: "none" | "relu" | "silu" | "gelu".  row_stats: the launch also writes cvmi_conv_desc.row_stats, per row and
    96-column slice (mean, sum of squared deviations) of the values stored (gemm256x192_kernel<float> / gemm256x192r_kernel only)."""
    return dict(id=rid, expect=expect, dtypes=dtypes, B=B, Cin=Cin, up=up, H=H, W=W, Cout=Cout, k=k, stride=stride,
                pad=k // 2 if pad is None else pad, out_hw=out_hw, act=act, res=res, res_rep=res_rep, act_after_res=act_after_res,
                shuffle_cout=shuffle_cout, out_f32=out_f32, y_pad=y_pad, scalar_gather=scalar_gather, row_stats=row_stats, note=note)


def conv_expect(row, dt):
    """The tag row `row` must report in dtype dt."""
    e = row["expect"]
    return (e[dt] if isinstance(e, dict) else e).replace("{T}", TNAME[dt])


CONV_ROWS = [
    # ================= conv_tile_kernel (fp16 and f32 builds; bf16 has no such path and takes igemm_kernel) =================
    # ---- 3x3 stride 1: CC 32 / 16 / 8, tile forms 32/8, 64/4, 64/8, 128/8
    _conv("t31_c32_n32", dict(f16=tile(3, 1, 32, 32), f32=tile(3, 1, 32, 32), bf16=ig(T128x32, 64, False)), 2, 32, 9, 21, 32, 3, dtypes=ALL3, act="silu",
          note="OW = 21: a second tile column with 5 of 16 pixels"),
    _conv("t31_c32_n64_res", dict(f16=tile(3, 1, 32, 64, 4), f32=tile(3, 1, 16, 64), bf16=ig(T64x64, 64, False)), 2, 32, 17, 13, 64, 3, dtypes=ALL3,
          act="silu", res="full", note="odd size; f32 cannot hold a 32-channel chunk next to 64 weight rows in LDS: CC = 16"),
    _conv("t31_c32_4chunks", dict(f16=tile(3, 1, 32, 64, 4), f32=tile(3, 1, 16, 64)), 1, 128, 12, 20, 64, 3, dtypes=F16_F32, act="relu",
          note="128 channels: the most conv_tile takes at stride 1; 4 (f32: 8) staged chunks"),
    _conv("t31_c32_n64_th8", dict(f16=tile(3, 1, 32, 64), f32=tile(3, 1, 16, 64)), 65, 32, 16, 32, 64, 3, dtypes=F16_F32, act="silu",
          note="260 tiles of 8 x 16 > 256: the 8-row form in fp16"),
    _conv("t31_c16_n24", dict(f16=tile(3, 1, 16, 32), f32=tile(3, 1, 16, 32), bf16=ig(T128x32, 64, False)), 1, 16, 20, 20, 24, 3, dtypes=ALL3,
          act="silu", y_pad=8),
    _conv("t31_c16_n128", dict(f16=tile(3, 1, 16, 128), f32=ig(T64x128, 64, False)), 1, 64, 10, 18, 128, 3, dtypes=F16_F32, act="silu", res="full", y_pad=8,
          note="fp16: 128 weight rows leave no room for CC = 32; f32: no chunk width fits -> igemm_kernel"),
    _conv("t31_c8_n16", dict(f16=tile(3, 1, 8, 32), f32=tile(3, 1, 8, 32), bf16=ig(T128x32, 64, False)), 3, 8, 9, 7, 16, 3, dtypes=ALL3,
          note="fp16 CC = 8: two taps per MFMA k-step, the tenth tap is a zero weight"),
    _conv("t31_c8_n96", tile(3, 1, 8, 128), 1, 24, 12, 20, 96, 3, dtypes=F16_F32, act="relu", res="full", note="3 chunks of 8 channels; N = 96 of a 128 tile"),
    # ---- 3x3 stride 2
    _conv("t32_c32_n32", dict(f16=tile(3, 2, 32, 32), f32=tile(3, 2, 16, 32), bf16=ig(T128x32, 64, False)), 1, 32, 20, 24, 32, 3, 2, dtypes=ALL3, act="silu"),
    _conv("t32_c16_n128", dict(f16=tile(3, 2, 16, 128), f32=ig(T64x128, 64, False), bf16=ig(T64x128, 64, False, 2)), 1, 64, 32, 32, 128, 3, 2, dtypes=ALL3,
          act="silu", note="64 channels: the most conv_tile takes at stride 2; bf16: 18 K-tiles on a 64 x 128 tile -> 2 K groups"),
    _conv("t32_c16_n40", dict(f16=tile(3, 2, 16, 64, 4), f32=ig(T64x64, 64, False)), 2, 16, 17, 33, 40, 3, 2, dtypes=F16_F32, act="relu", res="full", y_pad=8,
          note="odd H and W at stride 2: the last row / column sees 2 of 3 taps; f32: no chunk width fits next to 64 weight rows"),
    _conv("t32_c8_n48", dict(f16=tile(3, 2, 8, 64, 4), f32=tile(3, 2, 8, 64), bf16=ig(T64x64, 64, False)), 1, 24, 21, 19, 48, 3, 2, dtypes=ALL3, act="silu",
          note="odd H and W"),
    # ---- 2x2 stride 1 (pad 1: OH = H + 1)
    _conv("t21_c32_n32", tile(2, 1, 32, 32), 1, 32, 12, 12, 32, 2, dtypes=F16_F32, act="silu"),
    _conv("t21_c16_n128", tile(2, 1, 16, 128), 1, 48, 8, 15, 72, 2, dtypes=F16_F32, act="relu", note="N = 72: one vector over 64 -> the 128 tile"),
    _conv("t21_c8_n56", dict(f16=tile(2, 1, 8, 64, 4), f32=tile(2, 1, 8, 64), bf16=ig(T64x64, 64, False)), 2, 8, 9, 16, 56, 2, dtypes=ALL3, pad=0,
          note="pad 0: OW = 15; N = 56: one vector under 64"),
    _conv("t31_c16_n22_tail_res", tile(3, 1, 16, 32), 1, 16, 9, 7, 22, 3, dtypes=F16_F32, act="relu", res="full",
          note="N = 22: the ragged channel tail of conv_tile's epilogue (6 of 8 fp16 / 2 of 4 f32 elements), with a residual"),
    # ---- just outside conv_tile: igemm_kernel takes over
    _conv("k1224_ragged_group", dict(f16=ig(T64x128, 64, False, 2), bf16=ig(T64x128, 64, False, 2), f32=ig(T64x128, 64, False)), 1, 136, 19, 21, 72, 3,
          dtypes=ALL3, act="relu", res="full", note="3x3 s1 over 136 channels; K = 1224 -> 39 K-tiles over 2 groups (20 + 19)"),
    _conv("s2_72ch", dict(f16=ig(T64x64, 64, False, 2), bf16=ig(T64x64, 64, False, 2), f32=ig(T64x64, 64, False)), 2, 72, 20, 20, 64, 3, 2, dtypes=ALL3,
          act="silu", note="3x3 s2 over 72 channels; 21 K-tiles: 2 K groups on BN = 64"),
    _conv("n136_small", ig(T64x128, 64, False), 1, 16, 12, 12, 136, 3, dtypes=ALL3, act="silu", note="N = 136 > 128, one vector over the tile"),
    _conv("n136_big", ig(T128x128, 64, False), 2, 16, 128, 128, 136, 3, dtypes=ALL3, act="relu", note="the same at M = 32768: 512 tiles of 128 x 128"),
    _conv("cin12_f32", ig(T128x32, 64, False), 1, 12, 9, 7, 16, 3, dtypes=("f32",), note="12 channels: vectors of 4 but no conv_tile chunk width"),
    _conv("cin12_scalar", ig(T128x32, 64, False), 1, 12, 9, 7, 16, 3, scalar_gather=True, note="16-bit: per-element gather"),
    _conv("stem_cin3", ig(T128x32, 64, False), 2, 3, 32, 48, 16, 3, 2, dtypes=ALL3, act="silu", scalar_gather=True, note="K = 27"),

    # ================= igemm_kernel: tiles x (T, TO), BKB, PLAIN, KS =================
    # ---- N <= 32
    _conv("n32_m256", dict(f16=ig(T256x32, 128, True), bf16=ig(T256x32, 128, True), f32=ig(T256x32, 64, True)), 1, 16, 3, 43691, 32, dtypes=ALL3, act="silu",
          note="M = 131073: one row in the last 256-row tile"),
    _conv("n32_m256_f32out", ig(T256x32, 128, True, to="float"), 8, 16, 128, 130, 24, res="full", out_f32=True, y_pad=4),
    _conv("n32_m129", dict(f16=ig(T128x32, 128, True), bf16=ig(T128x32, 128, True), f32=ig(T128x32, 64, True)), 1, 16, 3, 43, 32, dtypes=ALL3, act="silu",
          res="full", note="M = 129"),
    _conv("n32_m127_f32out", ig(T128x32, 64, True, to="float"), 1, 72, 1, 127, 28, act="gelu", res="bcast", out_f32=True, note="M = 127; N one f32 vector under 32"),
    # ---- N <= 64
    _conv("n64_m128", dict(f16=ig(T128x64, 128, True), bf16=ig(T128x64, 128, True), f32=ig(T128x64, 64, True)), 8, 64, 100, 90, 64, dtypes=ALL3, act="silu"),
    _conv("n64_m128_f32out", ig(T128x64, 128, True, to="float"), 8, 64, 100, 90, 60, act="relu", res="full", out_f32=True, y_pad=4, note="N = 60: one f32 vector under 64"),
    _conv("n62_logits", ig(T64x64, 64, True), 1, 128, 40, 40, 62, dtypes=ALL3, note="ragged Cout: element-wise channel tail"),
    _conv("n62_tail_res_aar", ig(T64x64, 64, True), 1, 128, 40, 40, 62, dtypes=ALL3, act="relu", res="full", act_after_res=True,
          note="the element-wise channel tail with a residual and the activation after it"),
    _conv("n48_k64", dict(f16=ig(T64x64, 128, True), bf16=ig(T64x64, 128, True), f32=ig(T64x64, 64, True)), 1, 64, 5, 13, 48, dtypes=ALL3, act="relu", res="full",
          note="M = 65; K is exactly one 128-byte tile in 16 bits"),
    _conv("n64_f32out", ig(T64x64, 64, True, to="float"), 1, 96, 7, 9, 64, res="full", out_f32=True, note="M = 63"),
    # ---- 16-bit in, f32 out, N <= 192: 128 x 64 tiles
    _conv("f32out_n96", ig(T128x64, 128, True, to="float"), 2, 64, 8, 8, 96, res="full", out_f32=True),
    _conv("patch_embed", dict(f16=ig(T128x64, 64, False, to="float"), bf16=ig(T128x64, 64, False, to="float"), f32=ig(T64x128, 64, False)), 2, 48, 16, 16, 144, 2,
          dtypes=ALL3, pad=1, out_hw=(16, 16), res="bcast", out_f32=True, note="Hiera patch embedding: 2x2 over space-to-depth, out_hw crops the 17th row / column"),
    # ---- N > 64
    _conv("n160_big", dict(f16=ig(T128x128, 128, True), bf16=ig(T128x128, 128, True), f32=glds(64)), 8, 64, 100, 90, 160, dtypes=ALL3, act="silu",
          note="K = 64: too short for gemm_glds_kernel in 16 bits"),
    _conv("n72_deep_k", ig(T128x128, 128, True), 16, 1024, 64, 64, 72, dtypes=ALL3, act="relu", note="N < 96 keeps a deep plain GEMM on igemm_kernel; 128-byte K-tiles"),
    _conv("n200_f32out_big", ig(T128x128, 128, True, to="float"), 8, 64, 64, 64, 200, res="full", out_f32=True, y_pad=4),
    _conv("n200_f32out_small", ig(T64x128, 64, True, to="float"), 2, 96, 12, 10, 200, act="gelu", res="full", out_f32=True),
    _conv("n432_small", dict(f16=ig(T64x128, 64, True), bf16=ig(T64x128, 64, True), f32=ig(T64x128, 64, True)), 1, 144, 16, 16, 432, dtypes=ALL3, act="gelu",
          note="Hiera-like linear: 4 column tiles, the last one 48 wide"),
    # ---- split-K (16-bit, 64-row tiles)
    _conv("ks4_3x3", dict(f16=ig(T64x64, 64, False, 4), bf16=ig(T64x64, 64, False, 4), f32=ig(T64x64, 64, False)), 2, 256, 20, 20, 64, 3, dtypes=ALL3, act="silu",
          note="Detect cv2: 72 K-tiles"),
    _conv("ks4_plain", dict(f16=ig(T64x64, 64, True, 4), bf16=ig(T64x64, 64, True, 4), f32=ig(T64x64, 128, True)), 1, 1096, 10, 10, 40, dtypes=ALL3,
          note="35 K-tiles over 4 groups (9, 9, 9, 8)"),
    _conv("ks2_plain_n64", ig(T64x64, 64, True, 2), 1, 384, 10, 10, 48, act="silu", res="full", y_pad=8),
    _conv("ks2_plain_n128", dict(f16=ig(T64x128, 64, True, 2), bf16=ig(T64x128, 64, True, 2), f32=ig(T64x128, 64, True)), 3, 384, 20, 20, 128, dtypes=ALL3, act="silu"),
    _conv("ks2_two_sources", ig(T64x128, 64, False, 2), 2, (256, 128), 20, 20, 128, 3, up=0, act="silu", note="upsampled + skip, deep K: the gather restarts per group"),
    # ---- two sources
    _conv("two_src_generic", ig(T64x64, 64, False), 2, (32, 16), 12, 10, 40, dtypes=ALL3, up=0, act="silu", y_pad=16),
    _conv("rows2_up_first", ig(T64x128, 64, False), 3, (128, 64), 18, 22, 96, dtypes=ALL3, up=0, act="silu", note="two-row-pointer gather below 512 tiles"),
    _conv("rows2_up_second", ig(T64x128, 64, False), 3, (64, 128), 18, 22, 96, dtypes=ALL3, up=1, act="silu"),
    # ---- epilogue options on igemm_kernel
    _conv("ig_bcast", ig(T64x128, 64, True), 3, 256, 8, 8, 256, dtypes=ALL3, res="bcast", note="the decoder's positional tables"),
    _conv("ig_rep_mod", dict(f16=ig(T64x128, 128, True), bf16=ig(T64x128, 128, True), f32=ig(T64x128, 64, True)), 6, 64, 6, 5, 72, dtypes=ALL3, res="rep", res_rep=3, note="res_rep with res_mod = OH * OW"),
    _conv("ig_shuffle_rep_aar", dict(f16=ig(T64x128, 128, True), bf16=ig(T64x128, 128, True), f32=ig(T64x128, 64, True)), 6, 64, 6, 5, 128, dtypes=ALL3, act="gelu", res="rep", res_rep=3, act_after_res=True, shuffle_cout=32, y_pad=8,
          note="ConvTranspose 2x2 / s2 scatter + the skip feature shared by 3 prompts + GELU after it"),
    _conv("ig_rep_aar_n136", dict(f16=ig(T64x128, 128, True), bf16=ig(T64x128, 128, True), f32=ig(T64x128, 64, True)), 6, 64, 6, 5, 136, dtypes=ALL3, act="relu", res="rep", res_rep=3,
          act_after_res=True, note="column tile 0 is full: res_rep and the activation after it through the PREFETCHED residual; tile 1 is one 16-bit vector wide"),
    _conv("ig_aar", dict(f16=ig(T64x64, 128, True), bf16=ig(T64x64, 128, True), f32=ig(T64x64, 64, True)), 2, 32, 9, 7, 40, dtypes=ALL3, act="relu", res="full", act_after_res=True),

    # ================= gemm_glds_kernel: >= 512 tiles, K in whole 128-byte tiles (or >= 256) =================
    _conv("glds64", glds(64), 16, 128, 64, 64, 96, dtypes=ALL3, act="silu"),
    _conv("glds64_f32out", glds(64, to="float"), 16, 128, 64, 64, 100, act="relu", res="full", out_f32=True, y_pad=4, note="N = 100: one f32 vector over 96"),
    _conv("glds128_n648", glds(128), 1, 128, 27, 403, 648, dtypes=ALL3, act="gelu", note="M = 10881 = 85 x 128 + 1; N = 5 x 128 + 8"),
    _conv("glds128_f32out", glds(128, to="float"), 1, 128, 27, 403, 644, res="bcast", out_f32=True),
    _conv("glds64_ragged_k", glds(64), 16, 264, 64, 64, 96, act="relu", res="full", y_pad=8, note="K = 264: K % 64 = 8"),
    _conv("glds64_bcast", glds(64), 16, 128, 64, 64, 120, res="bcast", note="N = 120: one vector under 128"),
    _conv("glds64_shuffle_rep_aar", glds(64), 8, 128, 64, 64, 256, act="gelu", res="rep", res_rep=4, act_after_res=True, shuffle_cout=64, y_pad=8,
          note="the decoder's transposed conv at B = 2 images x 4 prompts"),
    _conv("glds_rows2_up_first", glds(64), 4, (64, 64), 128, 128, 96, up=0, act="silu"),
    _conv("glds_rows2_up_second", glds(64), 4, (64, 64), 128, 128, 96, up=1, act="silu", res="full"),
    # ---- one condition short of the 256-row kernels
    _conv("g256_255_tiles", glds(64), 255, 128, 16, 16, 256, act="silu", note="255 tiles of 256 x 256"),
    _conv("g256_col_eff", glds(64), 128, 128, 16, 16, 408, res="full", note="N = 408: 79.7 % of two 256-column tiles"),
    _conv("g192_k960", glds(64), 128, 960, 16, 16, 384, act="gelu", note="K = 960 < 1024"),
    _conv("g256_k64", ig(T128x128, 128, True), 256, 64, 16, 16, 256, act="silu", note="K = 64 < 128"),

    # ================= the 256-row DMA kernels (16-bit operands) =================
    _conv("g256_res", G256, 256, 128, 16, 16, 256, act="silu", res="full", y_pad=8, note="a residual keeps it off the persistent form"),
    _conv("g256_bcast_aar", G256, 256, 128, 16, 16, 256, act="relu", res="bcast", act_after_res=True),
    _conv("g256_f32out", G256_F32, 256, 128, 16, 16, 256, res="full", out_f32=True, y_pad=4),
    _conv("g256p", G256P, 256, 128, 16, 16, 256, act="gelu"),
    _conv("g256p_ypad_ragged", G256P, 256, 192, 16, 16, 440, act="silu", y_pad=8, note="512 tiles over 256 workgroups; N = 440 of 512; 3 K-tiles"),
    _conv("i2c", G256_I2C, 2, 64, 128, 128, 256, 3, act="silu", note="128 tiles, one K-tile per tap"),
    _conv("i2c_s2_odd_res", G256_I2C, 2, 64, 255, 257, 256, 3, 2, act="relu", res="full", y_pad=8, note="stride 2 on odd sizes"),
    _conv("i2c_ragged_m", G256_I2C, 2, 64, 127, 129, 256, 3, act="relu", res="full", note="M = 32766: the last of 128 row blocks is two rows short"),
    _conv("i2c_f32out", G256_I2C_F32, 2, 64, 128, 128, 256, 3, res="full", out_f32=True),
    _conv("i2c_127_tiles", ig(T64x128, 64, False), 2, 64, 127, 128, 256, 3, act="silu", note="127 tiles: one short; 508 tiles of 128 x 128 -> 64-row tiles"),
    _conv("g192_16", G192, 128, 1024, 16, 16, 384, act="gelu", y_pad=8),
    _conv("g192_16_res_bcast", G192, 128, 1024, 16, 16, 384, res="bcast"),
    _conv("g192_16_aar", G192, 128, 1024, 16, 16, 384, act="relu", res="full", act_after_res=True),
    _conv("g192_f32_act", G192_F32, 128, 2304, 16, 16, 384, act="relu", res="full", out_f32=True, note="gemm256x192r's shape with an activation"),
    _conv("g192_f32_bcast", G192_F32, 128, 1024, 16, 16, 384, res="bcast", out_f32=True),
    _conv("g192_f32_stats_ragged", G192_F32, 180, 1024, 16, 17, 384, res="full", out_f32=True, row_stats=True,
          note="M = 48960 = 191 x 256 + 64: the last row block misses the direct epilogue and takes the LDS one, statistics included (the others: direct)"),
    _conv("g192r", G192R, "cu/2", 2304, 16, 16, 384, res="full", out_f32=True, y_pad=4, note="CU-count tiles of 256 x 192: whole rounds; skipped unless CUs % 8 == 0"),
]

# dual-built entry point -> (test module, test function) that checks its bf16 build op by op
BF16_OPS = {
    "cvmi_attention": ("test_attention_matrix_gpu.py", "test_attention_matrix"),
    "cvmi_conv2d": ("test_conv_matrix_gpu.py", "test_conv_matrix"),            # (tests/test_bf16_ops_gpu.py test_conv2d_bf16* remain beside it)
    "cvmi_layernorm": ("test_helper_matrix_gpu.py", "test_layernorm_matrix"),      # (tests/test_bf16_ops_gpu.py test_layernorm_bf16 remains beside it)
    "cvmi_layernorm_dual": ("test_helper_matrix_gpu.py", "test_layernorm_dual_matrix"),
    "cvmi_maxpool2x2": ("test_bf16_ops_gpu.py", "test_maxpool_and_space_to_depth_bf16"),
    "cvmi_space_to_depth4": ("test_bf16_ops_gpu.py", "test_maxpool_and_space_to_depth_bf16"),
    "cvmi_cast": ("test_bf16_ops_gpu.py", "test_cast_bf16"),
    "cvmi_nchw_to_nhwc": ("test_bf16_ops_gpu.py", "test_nchw_to_nhwc_bf16"),
    "cvmi_prompt_tokens": ("test_bf16_ops_gpu.py", "test_prompt_tokens_bf16"),
    "cvmi_hyper_masks": ("test_bf16_ops_gpu.py", "test_hyper_masks_bf16"),
    "cvmi_hiera_mlp": ("test_ops_gpu.py", "test_hiera_mlp_fused_vs_torch"),
    "cvmi_tok_linear": ("test_ops_gpu.py", "test_tok_linear_vs_torch"),          # (its statistics and pool forms: test_tok_linear_forwarded_layernorm_statistics, test_tok_linear_pool_vs_torch)
    "cvmi_tok_linear16_launch": ("test_ops_gpu.py", "test_tok_linear16_row_blocks_shared_between_workgroups"),
    "cvmi_tok_linear16_splits": ("test_ops_gpu.py", "test_tok_linear16_row_blocks_shared_between_workgroups"),
    "cvmi_tok_linear16_shares": ("test_ops_gpu.py", "test_tok_linear16_row_blocks_shared_between_workgroups"),
}


# ---- the fused YOLO11 kernels: c3k2_fused.hip, stem_fused.hip, dwpw_fused.hip ----------------------------------------------------------------
C3K2_INSTANCES = ((16, 8, 64, 32), (32, 16, 128, 64), (16, 8, 64, 0), (32, 16, 64, 0), (32, 16, 128, 0))      # c3k2_kernel<C, HR, C2, C1>
C3K2_TILE = (8, 16)                                                                                         # output pixels of one workgroup tile


def c3k2_tag(inst):
    return "c3k2_kernel<%d, %d, %d, %d>" % inst


def c3k2_max_wgs_per_cu(inst):
    """Hardware ceiling of resident workgroups per CU (8 waves per SIMD): 8 for the 256-thread instances (c = 16), 4 for the 512-thread ones."""
    return 8 if inst[0] == 16 else 4


def dwpw_tag(cc, nchunk, n1p, n2p):
    return "dwpw_kernel<%d, %d, %d, %d>" % (cc, nchunk, n1p, n2p)


def _c3(suffix, inst, B, H, W, shortcut=1, x_off=0, x_extra=0, y_guard=0, note=""):
    """One cvmi_c3k2 launch on an NHWC [B, H, W, C1 or 2 C] input.  B = "persist": chosen on the device so that EVERY workgroup of the persistent
    grid runs at least two tiles and the tiles do not divide evenly (test_fused_matrix_gpu.persistent_batch; k = the ceiling above).  x_off /
    x_extra: the input sits at channel x_off of a buffer x_extra channels wider; y_guard: zeroed channels on both sides of the output."""
    return dict(kernel="c3k2", id="c3k2_%d_%d_%d_%d_%s" % (inst + (suffix,)), expect=c3k2_tag(inst), inst=inst, B=B, H=H, W=W, shortcut=shortcut,
                x_off=x_off, x_extra=x_extra, y_guard=y_guard, k=c3k2_max_wgs_per_cu(inst) if B == "persist" else 0, note=note)


def _st(rid, H2, W2, B=2, x_ld=16, y_guard=0, note=""):
    """One cvmi_stem2 launch on the space-to-depth(2) grid [B, H2, W2, 16 of x_ld] of a [B, 3, 2 H2, 2 W2] image."""
    return dict(kernel="stem2", id="stem2_" + rid, expect="stem2_kernel", B=B, H=H2, W=W2, x_off=0, x_extra=x_ld - 16, y_guard=y_guard, note=note)


def _dw(rid, expect, C, N1, N2, H=9, W=17, B=2, x_off=0, x_extra=0, y_guard=0, note=""):
    """One cvmi_dwpw launch: depthwise 3x3 over C channels, pointwise to N1, chained class conv to N2 (0 = none)."""
    return dict(kernel="dwpw", id="dwpw_" + rid, expect=expect, C=C, N1=N1, N2=N2, B=B, H=H, W=W, x_off=x_off, x_extra=x_extra, y_guard=y_guard, note=note)


FUSED_ROWS = []
for _inst in C3K2_INSTANCES:
    FUSED_ROWS += [
        _c3("8x16", _inst, 3, 8, 16, note="one whole tile: every halo pixel is outside the image"),
        _c3("1x1", _inst, 3, 1, 1, y_guard=8),
        _c3("7x15", _inst, 3, 7, 15, note="one row and column short of a tile"),
        _c3("9x17", _inst, 3, 9, 17, note="one pixel into a second tile row and column: both halos partly outside on every side"),
        _c3("19x37", _inst, 2, 19, 37, x_off=8, x_extra=16, y_guard=8, note="3 x 3 tiles, one interior; last row 3 of 8, last column 5 of 16"),
        _c3("9x17_noshort", _inst, 3, 9, 17, shortcut=0),
        _c3("persist", _inst, "persist", 19, 37, note="the persistent tile loop: prefetch, pmask, patch landing over the output tile"),
    ]
FUSED_ROWS += [
    _st("16x32", 16, 32, note="exactly one tile: halo column 32 is outside"),
    _st("1x1", 1, 1, B=3),
    _st("15x31", 15, 31, note="odd grid one short of a tile: OH = 8, OW = 16"),
    _st("17x33", 17, 33, note="odd grid one past a tile: OH = 9, OW = 17"),
    _st("21x27_ld24", 21, 27, x_ld=24),
    _st("34x66_guard", 34, 66, y_guard=8, note="OH = 17, OW = 33: 3 x 3 tiles"),
    # ---- dwpw: the eight instances by tag
    _dw("c64_n64", dwpw_tag(64, 1, 64, 0), 64, 64, 0),
    _dw("c128_n64", dwpw_tag(64, 2, 64, 0), 128, 64, 0),
    _dw("c256_n64", dwpw_tag(64, 4, 64, 0), 256, 64, 0),
    _dw("c64_n80", dwpw_tag(64, 1, 96, 0), 64, 80, 0),
    _dw("c128_n80", dwpw_tag(64, 2, 96, 0), 128, 80, 0, y_guard=8),
    _dw("c256_n96", dwpw_tag(64, 4, 96, 0), 256, 96, 0),
    _dw("c64_n64_cls62", dwpw_tag(64, 1, 64, 64), 64, 64, 62, note="ragged channel tail: 62 of 64"),
    _dw("c80_n80_cls62", dwpw_tag(80, 1, 96, 64), 80, 80, 62, y_guard=8),
    # ---- widths, sizes, layout
    _dw("n1_8", dwpw_tag(64, 1, 64, 0), 64, 8, 0, y_guard=8),
    _dw("cls64", dwpw_tag(64, 1, 64, 64), 64, 64, 64),
    _dw("cls8", dwpw_tag(80, 1, 96, 64), 80, 80, 8),
    _dw("1x1", dwpw_tag(64, 2, 96, 0), 128, 80, 0, H=1, W=1, B=3),
    _dw("8x16", dwpw_tag(64, 4, 64, 0), 256, 64, 0, H=8, W=16, note="one whole tile"),
    _dw("19x37_xoff", dwpw_tag(64, 2, 64, 0), 128, 64, 0, H=19, W=37, x_off=8, x_extra=16, y_guard=8, note="3 x 3 tiles; input inside a wider buffer"),
]
del _inst

# mutant of tests/fused_ref.py -> ids of the rows that must catch it (tests/test_fused_ref_cpu.py)
FUSED_MUTANT_ROWS = {
    "t_from_padded_b": [r["id"] for r in FUSED_ROWS if r["kernel"] == "c3k2" and r["id"].endswith(("_9x17", "_1x1"))],
    "ab_bias_outside": [r["id"] for r in FUSED_ROWS if r["kernel"] == "c3k2" and r["inst"][3] and r["id"].endswith(("_9x17", "_1x1"))],
    "no_shortcut": [r["id"] for r in FUSED_ROWS if r["kernel"] == "c3k2" and r["id"].endswith("_9x17")],
    "always_shortcut": [r["id"] for r in FUSED_ROWS if r["kernel"] == "c3k2" and r["id"].endswith("_9x17_noshort")],
    "rows_bleed": [r["id"] for r in FUSED_ROWS if r["B"] != "persist" and (r["kernel"] != "stem2" or r["H"] % 2 == 0)],
    "stem_t_bias_outside": ["stem2_17x33"],
    "dw_first_chunk_taps": ["dwpw_c128_n64", "dwpw_c128_n80"],
}


# ---- cvmi_layernorm / cvmi_layernorm_dual: sam_ops.hip launch_ln ---------------------------------------------------------------------------
LN_G = (4, 8, 16, 32, 64)                    # lanes per row
LN_NCAND = (1, 2, 3, 5, 8, 9)                # slots per lane: the instances of CVMI_LN_SW
LN_MAX_CHUNKS = LN_G[-1] * LN_NCAND[-1]      # beyond: "layernorm: C=.. too wide"
# form -> (input type, output type, channels per slot, WD).  "16": the 16-bit operand type of the row's dtype (fp16 or bf16).
LN_FORMS = {
    "f32_f32": ("float", "float", 4, 1),
    "f32_16w": ("float", "16", 8, 2),        # C % 8 == 0 and y_ld % 8 == 0: two 16-byte loads, one 16-byte store per slot
    "f32_16n": ("float", "16", 4, 1),        # C % 8 == 4 or y_ld % 8 == 4
    "16_16": ("16", "16", 8, 1),
    "16_f32": ("16", "float", 8, 1),
}
LN_PAD = (5, 7, 8, 8)                        # pad = (H, W, Hp, Wp): rows are pixels of [*, 5, 7] images written into a [*, 8, 8] grid


def ln_pick(C, slot):
    """launch_ln's choice for C channels in slots of `slot`: (G, NCH, waste) with waste = G * NCH - C / slot idle slots.  For every G the first
    NCH that fits; among those the least waste, then the smaller NCH."""
    assert C > 0 and C % slot == 0, (C, slot)
    chunks = C // slot
    best = None
    for G in LN_G:
        for n in LN_NCAND:
            if G * n < chunks:
                continue
            waste = G * n - chunks
            if best is None or waste < best[2] or (waste == best[2] and n < best[1]):
                best = (G, n, waste)
            break
    if best is None:
        raise ValueError(f"layernorm: C={C} too wide")
    return best


def ln_reachable(ncand=LN_NCAND):
    """{(G, NCH): [chunk counts that select it]} over every width launch_ln accepts."""
    global LN_NCAND
    keep, out = LN_NCAND, {}
    LN_NCAND = tuple(ncand)
    try:
        for chunks in range(1, LN_G[-1] * max(ncand) + 1):
            G, n, _ = ln_pick(chunks, 1)
            out.setdefault((G, n), []).append(chunks)
    finally:
        LN_NCAND = keep
    return out


def ln_tag(form, nch, dt):
    ti, to, _, wd = LN_FORMS[form]
    return "layernorm_kernel<%s, %s, %d, %d>" % (TNAME[dt] if ti == "16" else ti, TNAME[dt] if to == "16" else to, nch, wd)


def _ln(form, C, rows, tag, act="none", inside=0, pad=None):
    """One cvmi_layernorm launch over `rows` rows of C channels.  inside = 8: input and output sit at column 8 of buffers 8 columns wider on both
    sides.  The narrow f32 -> 16-bit form with C % 8 == 0 gets 4 more output columns (y_ld % 8 == 4), or the dispatcher would take the wide form."""
    slot = LN_FORMS[form][2]
    G, nch, waste = ln_pick(C, slot)
    y_more = 4 if form == "f32_16n" and C % 8 == 0 else 0
    return dict(id="%s_g%d_n%d_c%d_%s" % (form, G, nch, C, tag), form=form, dtypes=("f32",) if form == "f32_f32" else F16_BF16, C=C, rows=rows, G=G,
                NCH=nch, waste=waste, act=act, x_off=inside, x_ld=C + 2 * inside, y_off=inside, y_ld=C + 2 * inside + y_more, pad=pad)


def _ln_rows():
    out = []
    reach = ln_reachable()
    for form, (_, _, slot, _) in LN_FORMS.items():
        for (G, n), chunks in sorted(reach.items()):                      # every reachable instance at its smallest C: two workgroups, the second partial
            out.append(_ln(form, chunks[0] * slot, 4 * 64 // G + 3, "min"))
        for G, n in ((8, 3), (64, 2)):                                    # Hiera's NCH = 3 and the one-row-per-wave G = 64 form
            full, short = reach[(G, n)][-1] * slot, reach[(G, n)][-2] * slot  # every slot busy / one idle slot
            wg = 4 * 64 // G
            out += [_ln(form, full, 1, "rows1"), _ln(form, full, wg - 1, "wg_minus1"), _ln(form, full, wg + 1, "wg_plus1"),
                    _ln(form, short, wg + 3, "waste"), _ln(form, full, wg + 3, "inside", inside=8),
                    _ln(form, full, 3 * LN_PAD[0] * LN_PAD[1], "padgrid", pad=LN_PAD), _ln(form, full, wg + 3, "gelu", act="gelu")]
    # the narrow f32 -> 16-bit form by both of its conditions, at a Hiera-like width
    out += [_ln("f32_16n", 100, 67, "c_mod8_4"), _ln("f32_16n", 96, 67, "yld_mod8_4")]
    return out


LN_ROWS = _ln_rows()
# cvmi_layernorm_dual: f32 in place + a 16-bit copy (y2_ld = C + 8), NCH in {1, 3, 9}
LN_DUAL_ROWS = [dict(id="dual_c%d" % C, C=C, rows=67, dtypes=F16_BF16, G=ln_pick(C, 4)[0], NCH=ln_pick(C, 4)[1], expect="layernorm_kernel<float, float, %d, 1>" % ln_pick(C, 4)[1])
                for C in (256, 96, 144)]

# mutant of tests/helper_ref.py -> ids of the rows that must catch it (tests/test_helper_ref_cpu.py)
LN_MUTANT_ROWS = {
    "ln_stats_over_slots": [r["id"] for r in LN_ROWS if r["waste"] > 0 and r["id"].endswith("_waste")],
    "ln_rows_shift_at_wg": [r["id"] for r in LN_ROWS if r["id"].endswith(("_wg_plus1", "_waste", "_gelu"))],
    "ln_pad_row_uses_w": [r["id"] for r in LN_ROWS if r["pad"]],
}


# ---- the other helper kernels -----------------------------------------------------------------------------------------------------------------
GRID_CAP_ITEMS = {"cast": 4096 * 256, "maxpool2x2": 4096 * 256, "space_to_depth4": 4096 * 256, "nchw_to_nhwc": 4096 * 256, "nhwc_to_nchw_f32": 4096 * 256,
                  "sppf_pool": 4096 * 256, "bilinear": 1024 * 256, "hyper_masks": 64 * 256, "repeat_images": 64 * 256}   # work items of one grid pass
SPPF_LDS_PIXELS = {"f16": 1024, "f32": 2048}                              # the largest H * W of sppf_pool_lds_kernel (two f32 planes in 64 KiB)


def _sppf(rid, dt, B, H, W, C, ld_extra=0):
    lds = H * W <= SPPF_LDS_PIXELS[dt]
    return dict(op="sppf_pool", id="sppf_%s_%s" % (rid, dt), dtypes=(dt,), expect=("sppf_pool_lds_kernel<%s>" if lds else "sppf_pool_kernel<%s>") % TNAME[dt],
                B=B, H=H, W=W, C=C, ld=4 * C + ld_extra)


REFINE_KS = (3, 5, 7, 11)                                                 # the reference's head: upsample_refine_fast_kernel


def _rf(rid, hw, HW, ks=REFINE_KS, y_shift=0, N=2):
    """cvmi_upsample_refine: [N, h, w] -> bilinear to [N, H, W] -> refinement branches ks.  y_shift: the output starts that many floats into its buffer."""
    fast = tuple(ks) == REFINE_KS and y_shift == 0
    return dict(op="refine", id="refine_" + rid, dtypes=("f32",), expect="upsample_refine_fast_kernel" if fast else "upsample_refine_kernel<4>", N=N,
                h=hw[0], w=hw[1], H=HW[0], W=HW[1], ks=tuple(ks), y_shift=y_shift)


def _dw(rid, dt, H, W, res, act, B=3, C=24):
    return dict(op="dwconv3x3", id="dw_%s_%s" % (rid, dt), dtypes=(dt,), expect="", B=B, H=H, W=W, C=C, res=res, act=act, x_off=8, x_extra=16, y_guard=8)


def _loop2(op, rid, **kw):
    return dict(op=op, id="%s_%s" % (op, rid), expect="", **kw)


def _helper_rows():
    rows = []
    for dt, c in (("f16", 16), ("f32", 8)):                                # >= two 16-byte channel chunks everywhere
        edge = (32, 32) if dt == "f16" else (32, 64)
        rows += [_sppf("1x1", dt, 2, 1, 1, c), _sppf("3x5", dt, 2, 3, 5, c, ld_extra=8), _sppf("1x20", dt, 2, 1, 20, c), _sppf("20x1", dt, 3, 20, 1, c),
                 _sppf("lds_limit", dt, 2, edge[0], edge[1], c), _sppf("past_lds_limit", dt, 2, edge[0] + 1, edge[1], c, ld_extra=8)]
    rows.append(_sppf("second_pass", "f16", 16, 40, 40, 328))              # 16 * 1600 * 41 = 1049600 chunk-pixels > 2^20
    for H, W in ((16, 64), (17, 65), (5, 7), (33, 62), (40, 96)):
        rows += [_rf("fast_%dx%d_identity" % (H, W), (H, W), (H, W)), _rf("fast_%dx%d_nonint" % (H, W), ((H + 2) // 3 + 1, (W + 2) // 3 + 2), (H, W))]
    rows += [_rf("fast_16x64_up4", (4, 16), (16, 64)), _rf("fast_40x96_up4", (10, 24), (40, 96)), _rf("fast_20x28_up4", (5, 7), (20, 28))]
    rows += [_rf("generic_ks357", (9, 14), (21, 37), ks=(3, 5, 7)), _rf("generic_ks1", (9, 14), (21, 37), ks=(1,)), _rf("generic_ks15", (9, 14), (21, 37), ks=(15,)),
             _rf("generic_ks357_identity", (17, 33), (17, 33), ks=(3, 5, 7)), _rf("generic_unaligned_out", (9, 14), (21, 37), y_shift=1),
             _rf("generic_unaligned_out_up4", (10, 24), (40, 96), y_shift=1)]
    for dt in ("f16", "f32"):
        for H in (1, 3):
            for W in (1, 2, 3, 4, 5, 9):
                rows += [_dw("%dx%d_res_silu" % (H, W), dt, H, W, 1, "silu"), _dw("%dx%d_plain" % (H, W), dt, H, W, 0, "none")]
    # ---- the second pass of every capped grid-stride loop, bit-exact
    for a, b in (("f32", "f16"), ("f16", "f32"), ("f32", "f32"), ("f16", "f16"), ("f32", "bf16"), ("bf16", "f32"), ("bf16", "bf16")):
        rows.append(_loop2("cast", "%s_%s" % (a, b), dtypes=(a,), dst=b, rows=1025, C=1024, x_ld=1032, y_ld=1032))
    for dt in ALL3:
        rows.append(_loop2("maxpool2x2", dt, dtypes=(dt,), B=2, H=2 * 258, W=2 * 256, C=32 if dt == "f32" else 64))     # 8 chunks per output pixel
        rows.append(_loop2("space_to_depth4", dt, dtypes=(dt,), B=2, H=4 * 363, W=4 * 362))
    for a, b in (("f32", "f16"), ("f32", "f32"), ("f16", "f16"), ("f16", "f32"), ("f32", "bf16"), ("bf16", "bf16"), ("bf16", "f32")):
        rows.append(_loop2("nchw_to_nhwc", "%s_%s" % (a, b), dtypes=(a,), dst=b, B=2, C=3, H=420, W=417, ld=8))
    for dt in F16_F32:
        rows.append(_loop2("nhwc_to_nchw_f32", dt, dtypes=(dt,), B=2, C=5, H=330, W=319, ld=8))
    rows.append(_loop2("repeat_images", "rep3", dtypes=("f32",), B=2, rep=3, chunks=64 * 256 + 37))
    rows.append(dict(op="bilinear", id="bilinear_520x517", dtypes=("f32",), expect="", N=2, h=130, w=97, H=520, W=517))
    rows.append(dict(op="mask_postprocess", id="mask_postprocess_520x517", dtypes=("f32",), expect="", N=2, h=130, w=97, H=520, W=517))
    for C, seed in ((32, 1), (64, 0)):
        rows.append(dict(op="hyper_masks", id="hyper_masks_c%d" % C, dtypes=ALL3, expect="", B=3, P=129 * 129, C=C, up_ld=C + 8, delta=0.05, thresh=0.98, seed=seed))
    return rows


HELPER_ROWS = _helper_rows()

HELPER_MUTANT_ROWS = {
    "sppf_clip_zero": [r["id"] for r in HELPER_ROWS if r["op"] == "sppf_pool" and "second_pass" not in r["id"]],
    "sppf_two_stages": [r["id"] for r in HELPER_ROWS if r["op"] == "sppf_pool" and max(r["H"], r["W"]) >= 20 and "second_pass" not in r["id"]],
    "refine_pad_before_upsample": [r["id"] for r in HELPER_ROWS if r["op"] == "refine" and (r["h"], r["w"]) != (r["H"], r["W"]) and max(r["ks"]) > 1],
    "refine_taps_transposed": [r["id"] for r in HELPER_ROWS if r["op"] == "refine" and max(r["ks"]) > 1],
    "dw_tail_reads_next_row": [r["id"] for r in HELPER_ROWS if r["op"] == "dwconv3x3" and r["H"] > 1],
}


# ---- the token-stationary path: tok_linear.hip, tok_linear16.hip, hiera_mlp.hip, tok_stream.hpp ------------------------------------------------
# TOK_ROWS: one row = one launch of cvmi_tok_linear (plain or pool form) and the instance its dispatcher must tag; MLP_ROWS: one
# launch of cvmi_hiera_mlp.  Tags carry no operand type: every row runs in fp16 and bf16.  Operands, references and the tolerance live in
# tests/tok_ref.py.  tok_pick / tl16_splits / mlp_pick mirror the host code (tests/test_op_coverage_cpu.py holds the mirror to the sources' text).
TOK_KS = (144, 288, 576)
TOK_FORMAT = {144: 32, 288: 32, 576: 16}          # cvmi_tok_linear_format: the MFMA shape of the packed weights
TOK_SLOTS = {32: 4, 16: 3}                         # weight ring depth (TlCfg / Tl16Cfg SLOTS); chunks are prefetched SLOTS - 1 ahead
_BOOL = {False: "false", True: "true"}


def tok_dispatch(ln, res, gelu):
    """tok_stream.hpp tok_dispatch: (LN, RES, GELU) of the instance for a LayerNorm-input / residual-output / GELU request."""
    if res:
        return (1, True, False) if ln else (0, True, False)
    if ln:
        return (1, False, True) if gelu else (1, False, False)
    return (0, False, True) if gelu else (0, False, False)


def tok_pick(K, ln, res, gelu, N, out_ld, pool=False):
    """The tag of the launch cvmi_tok_linear (pool: its pool form) ends in.  ln: 0 = 16-bit input, 1 = f32 + LayerNorm,
    2 = f32 converted as it is."""
    assert K in TOK_KS and ln in (0, 1, 2) and not (gelu and res) and (ln != 2 or not (res or gelu)), (K, ln, res, gelu)
    if TOK_FORMAT[K] == 16:
        assert ln != 2, "plain f32 input is built for K = 144 and 288"
        if pool:
            return "tok_linear16_kernel<%d, %d, %s, %s, %s>" % (K, 1, "false", "false", "true")
        assert res or (N % 8 == 0 and out_ld % 8 == 0), "16-bit output needs N and out_ld multiples of 8"
        LN, RES, GELU = tok_dispatch(ln != 0, res, gelu)
        return "tok_linear16_kernel<%d, %d, %s, %s, %s>" % (K, LN, _BOOL[RES], _BOOL[GELU], "false")
    if pool:
        return "tok_linear_kernel<%d, %d, %s, %s, %s, %s>" % (K, 1, "false", "false", "false", "true")
    LN, RES, GELU = (2, False, False) if ln == 2 else tok_dispatch(ln != 0, res, gelu)
    tstore = not RES and N % 8 == 0 and out_ld % 8 == 0                      # launch_tl
    return "tok_linear_kernel<%d, %d, %s, %s, %s, %s>" % (K, LN, _BOOL[RES], _BOOL[GELU], _BOOL[tstore], "false")


def tl16_splits(rows, N, stats_out):
    """tok_linear16.hip tl16_splits: workgroups that share one 256-row block of a K = 576 launch."""
    wg, nch = rows // 256, (N + 31) // 32
    if wg >= 256 or wg % 8 != 0 or (stats_out and N % 32 != 0):
        return 1
    best = 1
    for ns in range(2, 9):
        if ns <= nch and nch % ns == 0 and wg * ns <= 256:
            best = ns
    return best


def mlp_pick(C, pipe=None):
    """hiera_mlp.hip: C = 144 runs VAR 1, C = 288 VAR 2, or VAR 0 when the CVMI_MLP_PIPE test hook is set without bit 1."""
    assert C in (144, 288), C
    if C == 144:
        return "hiera_mlp_kernel<144, 1>"
    return "hiera_mlp_kernel<288, %d>" % (0 if pipe is not None and not (int(pipe) & 2) else 2)


def _tok_instances():
    out = set()
    for K in TOK_KS:
        out.add(tok_pick(K, 1, False, False, 32, 32, pool=True))
        for ln in (0, 1) + ((2,) if TOK_FORMAT[K] == 32 else ()):
            for res, gelu in ((False, False), (False, True), (True, False)):
                if ln == 2 and (res or gelu):
                    continue
                for N, out_ld in ((32, 32), (36, 40), (32, 36)):
                    if TOK_FORMAT[K] == 32 or res or (N % 8 == 0 and out_ld % 8 == 0):
                        out.add(tok_pick(K, ln, res, gelu, N, out_ld))
    return sorted(out)


TOK_INSTANCES = _tok_instances()                                            # 26 tok_linear_kernel + 7 tok_linear16_kernel
MLP_INSTANCES = sorted({mlp_pick(144), mlp_pick(288), mlp_pick(288, "0")})
TOK_PARTS = (2, 3, 6)                                                       # slice counts of the per-slice statistics rows, at every K
TOK_SPLIT_TABLE = ((2048, 64, 2), (2048, 96, 3), (2048, 160, 5), (2048, 224, 7), (2048, 256, 8), (2048, 576, 6), (2048, 544, 1), (2048, 40, 2),
                   (2304, 256, 1), (16384, 256, 4))                         # (rows, N, workgroups per row block) of the K = 576 split rows
# chunk counts every (K, family) needs: below the prefetch distance, equal to it, equal to SLOTS, one past SLOTS (the first reused slot), more
TOK_NCH = {32: (1, 2, 3, 4, 5, 9), 16: (1, 2, 3, 4, 7)}
TOK_NCH_FAMILIES = ("tstore", "direct", "res_ln0", "res_ln1")                # (K = 576 has no direct-store form: its 16-bit rows are all staged)


def _tok(tag, K, N, out_ld, ln=0, res=False, gelu=False, rows=256, grid=None, in_ld=None, stats_in=None, stats_out=False, row_off=0, fam="inst", chain=False):
    """One launch.  ln / res / gelu / grid (pool: (B, H, W)) are the form.  in_ld > K: the input's padding columns hold NaN.  out_ld > N: guard
    columns hold a sentinel.  stats_in: None, "pair" = forwarded (mean, rstd), or P = per-slice (mean, M2) pairs.  stats_out: the residual form
    also writes the updated rows' statistics.  row_off: the input is a view that many rows into a larger tensor.  chain: the statistics written are
    consumed by a second launch (tests/test_tok_matrix_gpu.py).  ns (K = 576): workgroups per row block, what tl16_splits must say."""
    pool = grid is not None
    if pool:
        rows, ln = grid[0] * grid[1] * grid[2], 1
    in_ld = K if in_ld is None else in_ld
    form = "pool" if pool else "ln%d%s%s" % (ln, "_res" if res else "", "_gelu" if gelu else "")
    rid = "k%d_%s_n%d_ld%d_%s" % (K, form, N, out_ld, tag)
    return dict(id=rid, fam=fam, expect=tok_pick(K, ln, res, gelu, N, out_ld, pool), K=K, N=N, rows=rows, grid=grid, in_ld=in_ld, out_ld=out_ld, ln=ln, res=res,
                gelu=gelu, pool=pool, stats_in=stats_in, stats_out=stats_out, row_off=row_off, chain=chain, dtypes=F16_BF16,
                ns=tl16_splits(rows, N, res and stats_out) if TOK_FORMAT[K] == 16 else None)


def tok_nch_family(r):
    """The chunk-count family a row belongs to ("tstore" | "direct" | "res_ln0" | "res_ln1"), or None."""
    if r["pool"] or r["ln"] == 2:
        return None
    if r["res"]:
        return "res_ln%d" % r["ln"]
    return "tstore" if r["N"] % 8 == 0 and r["out_ld"] % 8 == 0 else "direct"


def _tok_rows():
    out = []
    forms16 = ((0, False), (0, True), (1, False), (1, True))
    for K in TOK_KS:                                                        # ---- every instance, one workgroup
        f32fmt = TOK_FORMAT[K] == 32
        for ln, gelu in forms16 + (((2, False),) if f32fmt else ()):
            out.append(_tok("inst", K, 40, 48, ln=ln, gelu=gelu))            # staged store: two chunks, the last a single 8-column piece
            if f32fmt:
                out += [_tok("inst", K, 36, 40, ln=ln, gelu=gelu), _tok("inst", K, 32, 36, ln=ln, gelu=gelu)]      # direct store: by N, by the stride alone
        out += [_tok("inst", K, 44, 48, ln=ln, res=True) for ln in (0, 1)]
        out.append(_tok("inst", K, 36, 40, grid=(1, 16, 16)))
    for K in TOK_KS:                                                        # ---- chunk counts around the ring, ragged and whole last chunks
        f32fmt = TOK_FORMAT[K] == 32
        for N in (8, 32, 64, 96, 104, 128, 136, 160, 288) if f32fmt else (8, 32, 64, 96, 104, 128, 200, 224):
            out.append(_tok("nch", K, N, N + 8, ln=1, gelu=True, fam="nch"))
            if f32fmt:
                out.append(_tok("nch", K, N, N + 4, ln=0, fam="nch"))
            else:
                out.append(_tok("nch", K, N, N + 8, ln=0, fam="nch"))
            out += [_tok("nch", K, N, N + 4, ln=ln, res=True, fam="nch") for ln in (0, 1)]
        if f32fmt:                                                          # N = 144: the residual form's half chunk (tok_linear.hip, res_load)
            out += [_tok("nch", K, 144, 144, ln=ln, res=True, fam="nch") for ln in (0, 1)]
    for K in TOK_KS:                                                        # ---- layout: three workgroups, padded NaN input, guards, an offset view
        pad16, pad32 = K + 8, K + 4
        out += [_tok("layout", K, 72, 80, ln=0, gelu=True, rows=768, in_ld=pad16, row_off=256, fam="layout"),
                _tok("layout", K, 72, 80, ln=1, rows=768, in_ld=pad32, row_off=256, fam="layout"),
                _tok("layout", K, 68, 76, ln=1, res=True, rows=768, in_ld=pad32, row_off=256, stats_out=True, fam="layout"),
                _tok("layout", K, 68, 76, ln=0, res=True, rows=768, in_ld=pad16, row_off=256, stats_out=True, fam="layout")]
        if TOK_FORMAT[K] == 32:
            out += [_tok("layout", K, 72, 80, ln=2, rows=768, in_ld=pad32, row_off=256, fam="layout"),
                    _tok("layout", K, 68, 76, ln=1, gelu=True, rows=768, in_ld=pad32, row_off=256, fam="layout")]
    for K in TOK_KS:                                                        # ---- statistics out / in
        out += [_tok("stats", K, 136, 144, ln=0, res=True, stats_out=True, fam="stats"), _tok("stats", K, K, K, ln=0, res=True, stats_out=True, fam="stats"),
                _tok("stats", K, 136, 144, ln=1, res=True, stats_out=True, stats_in="pair", fam="stats"),
                _tok("pair", K, 72, 80, ln=1, gelu=True, stats_in="pair", fam="stats"), _tok("pair", K, 72, 80, ln=1, stats_in="pair", fam="stats")]
        out += [_tok("parts%d" % P, K, 72, 80, ln=1, stats_in=P, fam="stats") for P in TOK_PARTS]
        out.append(_tok("parts6", K, 68, 72, ln=1, res=True, stats_in=6, fam="stats"))
    K = 576                                                                 # ---- K = 576: row blocks shared between workgroups (gridDim.y > 1, j0 != 0)
    for rows, N, ns in TOK_SPLIT_TABLE:
        if rows == 2048:
            out.append(_tok("split%d" % ns, K, N, N + 8, ln=1, gelu=True, rows=rows, fam="split"))
        else:
            out.append(_tok("split%d_rows%d" % (ns, rows), K, N, N + 8, ln=0, rows=rows, fam="split"))
    out += [_tok("split3", K, 96, 100, ln=0, res=True, rows=2048, fam="split"), _tok("split2", K, 40, 44, ln=1, res=True, rows=2048, fam="split"),
            _tok("split6_parts_out", K, 576, 576, ln=0, res=True, rows=2048, stats_out=True, chain=True, fam="split"),
            _tok("split1_stats_out", K, 40, 44, ln=0, res=True, rows=2048, stats_out=True, fam="split"),
            _tok("split3", K, 96, 100, grid=(2, 32, 32), fam="split")]
    for K in TOK_KS:                                                        # ---- POOL grids: square, half width 3 with B > 1, wide, one pooled row
        for grid, N, ld in (((1, 16, 16), 64, 64), ((2, 64, 6), 36, 40), ((2, 64, 6), 64, 68), ((3, 8, 32), 36, 40), ((1, 2, 128), 64, 72)):
            out.append(_tok("grid%dx%dx%d" % grid, K, N, ld, grid=grid, fam="pool"))
        out.append(_tok("grid2x64x6_pair", K, 36, 40, grid=(2, 64, 6), stats_in="pair", in_ld=K + 4, fam="pool"))
    return out


TOK_ROWS = _tok_rows()
MLP_ROW_COUNTS = (1, 5, 31, 32, 33, 127, 128, 129, 391)                     # wave (32) and workgroup (128) boundaries; 391: the fourth workgroup's ragged tile


def _mlp(C, pipe, rows, stats_out=True, x_ld=None):
    x_ld = C + 4 if x_ld is None else x_ld
    tag = mlp_pick(C, pipe)
    return dict(id="mlp_c%d_v%s_rows%d_ld%d%s" % (C, tag[-2], rows, x_ld, "" if stats_out else "_nostats"), expect=tag, C=C, pipe=pipe, rows=rows, x_ld=x_ld,
                stats_out=stats_out, dtypes=F16_BF16)


MLP_ROWS = [_mlp(C, pipe, rows) for C, pipe in ((144, None), (288, None), (288, "0")) for rows in MLP_ROW_COUNTS] + \
           [_mlp(C, pipe, rows, stats_out=False) for C, pipe in ((144, None), (288, None), (288, "0")) for rows in (129, 391)] + \
           [_mlp(C, pipe, 391, x_ld=C) for C, pipe in ((144, None), (288, None), (288, "0"))]
# One 391-row launch per instance whose LayerNorm input carries the row kinds of tok_ref.mlp_operands (rows 500 away from zero, a ramp along C,
# a spread of 1e-3, an outlier in channel 0 -- the hand-over's shift -- and in the last channel, the rest plain).  Kept beside MLP_ROWS, whose
# operands and measured constant they do not touch.
MLP_KIND_ROWS = [dict(_mlp(C, pipe, 391), id="mlp_c%d_v%s_rows391_kinds" % (C, mlp_pick(C, pipe)[-2]), kinds=True) for C, pipe in ((144, None), (288, None), (288, "0"))]
KIND_ROWS = 32                                                              # rows per kind: one wave's token tile
KIND_BLOCKS = ("far500", "ramp", "spread1e-3", "outlier_c0", "outlier_last")  # rows [32 i, 32 i + 32) of a `kinds` launch


# ---- the proj + MLP launch: proj_mlp.hpp, the proj form of cvmi_hiera_mlp ---------------------------------------------------------------------
# PROJ_ROWS: one row = one launch of op_hiera_mlp(.., proj=..) and the instance proj_mlp_dispatch must tag.  x has a row stride of C + 4, ao of
# C + 8, both with NaN padding (the `tight` rows: C and C).  Operands, the reference, its mutants and the bound live in tests/tok_ref.py.
def proj_pick(C):
    """proj_mlp.hpp proj_mlp_dispatch: C = 144 runs the chunk-order loop (VAR 1), C = 288 the pipelined one (VAR 2)."""
    assert C in (144, 288), C
    return "proj_mlp_kernel<%d, %d>" % (C, 1 if C == 144 else 2)


PROJ_INSTANCES = sorted({proj_pick(144), proj_pick(288)})
PROJ_TODAY = ((144, 5), (144, 1000), (144, 128 * 3 + 37), (288, 5), (288, 777))   # the (C, rows) of tests/proj_mlp_cases.py before the matrix


def _proj(C, rows, stats_out=True, tight=False, kinds=False):
    x_ld, ao_ld = (C, C) if tight else (C + 4, C + 8)
    rid = "proj_c%d_rows%d_ld%d%s%s" % (C, rows, x_ld, "" if stats_out else "_nostats", "_kinds" if kinds else "")
    return dict(id=rid, expect=proj_pick(C), C=C, rows=rows, x_ld=x_ld, ao_ld=ao_ld, stats_out=stats_out, kinds=kinds, proj=True, pipe=None, dtypes=F16_BF16)


PROJ_ROWS = [_proj(C, rows) for C in (144, 288) for rows in MLP_ROW_COUNTS] + \
            [_proj(C, rows) for C, rows in PROJ_TODAY if rows not in MLP_ROW_COUNTS] + \
            [_proj(C, rows, stats_out=False) for C in (144, 288) for rows in (129, 391)] + \
            [_proj(C, 391, tight=True) for C in (144, 288)] + \
            [_proj(C, 391, kinds=True) for C in (144, 288)]


def _tok_ids(pred):
    return [r["id"] for r in TOK_ROWS if pred(r)]


def _nch(r):
    return (r["N"] + 31) // 32


# mutant of tests/tok_ref.py -> ids of the rows that must catch it, in every dtype of TOK_MUTANT_DTYPES[mutant] (default: both)
# (tests/test_tok_ref_cpu.py).  The predicates say where each mistake can show at all.
TOK_MUTANT_ROWS = {
    "ring_stale_slot": _tok_ids(lambda r: r["fam"] == "nch" and _nch(r) > TOK_SLOTS[TOK_FORMAT[r["K"]]]),
    "split_ring_origin": _tok_ids(lambda r: r["fam"] == "split" and (r["ns"] or 1) > 1),
    "last_piece_dropped": _tok_ids(lambda r: r["fam"] in ("nch", "inst") and r["N"] % 32 != 0),
    "guard_written": _tok_ids(lambda r: r["fam"] in ("nch", "inst", "layout") and r["N"] % 32 != 0 and r["out_ld"] > r["N"]),
    "res_overwrite": _tok_ids(lambda r: r["res"]),
    "ln_no_eps": _tok_ids(lambda r: r["ln"] == 1 and r["stats_in"] is None and r["fam"] in ("inst", "layout", "pool")),
    "ln_var_n_minus_1": _tok_ids(lambda r: r["ln"] == 1 and r["res"] and r["stats_in"] is None and r["fam"] in ("inst", "nch") and r["K"] == 144),
    "chan_no_between_term": _tok_ids(lambda r: isinstance(r["stats_in"], int)),
    "chan_raw_moments": _tok_ids(lambda r: isinstance(r["stats_in"], int)),
    "stats_over_ld": _tok_ids(lambda r: r["stats_out"] and r["out_ld"] > r["N"]),
    "pool_dxdy_swapped": _tok_ids(lambda r: r["pool"]),
    "pool_w_for_hw": _tok_ids(lambda r: r["pool"] and r["grid"][1] != r["grid"][2]),
    "pool_mean": _tok_ids(lambda r: r["pool"]),
    "bias_hi_only": _tok_ids(lambda r: r["res"] and r["ln"] == 0 and TOK_FORMAT[r["K"]] == 32 and r["fam"] in ("inst", "nch")),
    "mlp_rows_past_end": [r["id"] for r in MLP_ROWS if r["rows"] % 128 != 0],
}
# ln_var_n_minus_1: a 0.35 % change of rstd (K = 144) is below the bf16 step of the B fragments it feeds (2^-8); the f32 residual form sees it in fp16
TOK_MUTANT_DTYPES = {"ln_var_n_minus_1": ("f16",)}
# Mutants the fp64 comparison cannot see on any row, kept in tok_ref.py so that the CPU test records the blind spot with its measurement:
# mlp_hidden_not_rounded is MORE accurate than the contract by the rounding noise of 4 C hidden values, 0.09 (fp16) / 0.45 (bf16) of the MLP bound,
# which is set by the GELU form's error.
TOK_UNSEEN_MUTANTS = {"mlp_hidden_not_rounded": [r["id"] for r in MLP_ROWS if r["rows"] >= 127]}
# mutants of tok_ref.proj_mlp_ref -> ids of the PROJ_ROWS that must catch each, in fp16 and bf16.  The last three live where their kind of row
# is: raw moments cancel on rows 500 away from zero only, and x1 rounded to 16 bits is below the bound until x1 is large.
_PROJ_ALL, _PROJ_KINDS = [r["id"] for r in PROJ_ROWS], [r["id"] for r in PROJ_ROWS if r["kinds"]]
PROJ_MUTANT_ROWS = {
    "proj_bias_twice": _PROJ_ALL,
    "proj_bias_not_in_ln": _PROJ_ALL,
    "ln_of_x_not_x1": _PROJ_ALL,
    "residual_drops_proj": _PROJ_ALL,
    "fc1_k_natural_order": _PROJ_ALL,
    "proj_rows_past_end": [r["id"] for r in PROJ_ROWS if r["rows"] % 128 != 0],
    "stats_of_x1": [r["id"] for r in PROJ_ROWS if r["stats_out"]],
    "ln_var_raw_moments": _PROJ_KINDS,
    "stats_unshifted": _PROJ_KINDS,
    "x1_through_16_bits": _PROJ_KINDS,
}
# ... of tok_ref.hiera_mlp_ref on the MLP_KIND_ROWS
MLP_KIND_MUTANT_ROWS = {"ln_var_raw_moments": [r["id"] for r in MLP_KIND_ROWS], "stats_unshifted": [r["id"] for r in MLP_KIND_ROWS]}
# the mutants above that must show on the rows 500 away from zero (rows [0, KIND_ROWS) of a `kinds` launch)
FAR500_MUTANTS = ("ln_var_raw_moments", "stats_unshifted")


# ---- the detector's tail: vision_ops.hip cvmi_detect_decode, nms.hip cvmi_yolo_nms / cvmi_yolo_nms_best ---------------------------------------
# NMS_ROWS: one row = one input of nms_launch with an EXACT candidate count n per image (tests/detect_ref.py places exactly n best-class scores
# above conf_thres and some at exactly conf_thres), the instance it must tag and the decisions nms_pick -- a mirror of nms_launch and of the
# kernel's own branches -- derives from (A, n).  DECODE_ROWS: one row = one launch of cvmi_detect_decode per dtype.  Generators, references,
# mutants and the decode bound live in tests/detect_ref.py.
NMS_LDS_A, NMS_MAX_A, NMS_MAX_DET, NMS_MAX_NMS = 16384, 65536, 4096, 30000
NMS_NTHR_N = 2048                                  # up to this many candidates four waves run the passes, sixteen beyond
NMS_CAND_BYTES, NMS_WS_RECORD = 20, 28             # sizeof(Cand); workspace bytes per anchor (Cand + best score + best class)
NMS_KINDS = ("cluster", "isolated", "touch", "clsoff", "rounding", "maxnms")


def nms_pick(A, n):
    """(gk, P, Ps, nthr, geo_lds) of nms_launch / yolo_nms_kernel for A anchors of which n are candidates: keys in the workspace, key slots, sorted
    length, threads that stay after the candidate pass, geometry in LDS behind the sorted keys."""
    assert 0 < A <= NMS_MAX_A and 0 <= n <= A, (A, n)
    P = 1024
    while P < A:
        P <<= 1
    gk = A > NMS_LDS_A
    nthr = 256 if n <= NMS_NTHR_N else 1024
    Ps = 1
    while Ps < n:
        Ps <<= 1
    geo_lds = (not gk) and Ps * 8 + min(n, NMS_MAX_NMS) * NMS_CAND_BYTES <= P * 8
    return gk, P, Ps, nthr, geo_lds


def nms_workspace(B, A):
    """cvmi_yolo_nms_workspace: the records, 256 spare bytes, rounded up to 16, and the GK keys behind them."""
    P = nms_pick(A, 0)[1]
    return ((B * A * NMS_WS_RECORD + 256 + 15) & ~15) + (B * P * 8 if A > NMS_LDS_A else 0)


def nms_tag(gk):
    return "yolo_nms_kernel<%s>" % ("true" if gk else "false")


def _nms(rid, A, n, B=2, nc=4, conf=0.25, iou=0.7, max_det=300, max_wh=7680.0, kind="cluster", entry="best", clusters=12, jitter=1.5, zero=0.0,
         equal_scores=False, survivors=None, note=""):
    """entry: "best" = cvmi_yolo_nms_best alone, "both" = cvmi_yolo_nms as well (identical outputs).  kind: the box layout (detect_ref.nms_inputs).
    survivors: what the reference must find before max_det cuts the list ("==300", ">300", ..), asserted on the CPU."""
    gk, P, Ps, nthr, geo = nms_pick(A, n)
    return dict(id=rid, expect=nms_tag(gk), A=A, n=n, B=B, nc=nc, conf=conf, iou=iou, max_det=max_det, max_wh=max_wh, kind=kind, entry=entry,
                clusters=clusters, jitter=jitter, zero=zero, equal_scores=equal_scores, survivors=survivors, gk=gk, P=P, Ps=Ps, nthr=nthr, geo_lds=geo, note=note)


NMS_ROWS = [
    # ---- the six reachable (gk, nthr, geo_lds)
    _nms("lds_256_geo", 1024, 100, entry="both", note="A = 1024: the last A with P = 1024"),
    _nms("lds_1024_geo", 8193, 3000, note="P = 16384 at its smallest A"),
    _nms("lds_256_nogeo", 2100, 1500, entry="both"),
    _nms("lds_1024_nogeo", 2049, 2049, note="n = A = 2049: the first n with sixteen waves; Ps = P = 4096"),
    _nms("gk_256_odd", 16385, 500, B=3, entry="both", note="B * A odd: the workspace key offset is rounded up to 16 bytes"),
    _nms("gk_1024_b1", 16386, 2500, B=1, nc=62),
    # ---- n edges at the smallest A that holds them (and a few anchors at exactly conf_thres)
    _nms("n0", 5, 0, entry="both"), _nms("n1_a1", 1, 1, B=3, entry="both", note="A = 1"), _nms("n1", 5, 1), _nms("n2", 5, 2, entry="both"), _nms("n3", 7, 3, clusters=1),
    _nms("n255", 300, 255), _nms("n256_quarter_p1024", 300, 256, note="n = P / 4: the last n with the geometry in LDS"),
    _nms("n257_quarter_p1024_plus1", 300, 257, entry="both", note="Ps = 512: keys and geometry no longer fit"),
    _nms("n2047", 2100, 2047), _nms("n2048", 2100, 2048, note="the last n with four waves"), _nms("n2049_geo", 8193, 2049, note="sixteen waves, geometry in LDS"),
    _nms("n4096_quarter_p16384", 8193, 4096), _nms("n4097_quarter_p16384_plus1", 8193, 4097),
    _nms("full_1024", 1024, 1024, note="every anchor a candidate, every key slot used"), _nms("full_16384", 16384, 16384, nc=3, clusters=40, note="the last A with LDS keys, full"),
    # ---- A edges
    _nms("a1025", 1025, 200, note="P = 2048"), _nms("a65536_second_grid_pass", 65536, 50, B=17, nc=2, entry="both",
                                                    note="B * A > 4096 * 256: best_class_kernel's second grid pass; A = NMS_MAX_A"),
    # ---- max_det: the LDS list kept_pos and the loop bound
    _nms("md1", 300, 100, max_det=1, entry="both"),
    _nms("md300_exact", 400, 300, kind="isolated", survivors="==300"), _nms("md300_more", 500, 400, kind="isolated", survivors=">300", entry="both"),
    _nms("md4096_more", 4300, 4200, kind="isolated", max_det=4096, survivors=">4096", note="NMS_MAX_DET"),
    # ---- thresholds and degenerate geometry
    _nms("conf0", 300, 120, conf=0.0, entry="both", note="non-candidates score exactly 0"),
    _nms("iou0_touch", 330, 300, nc=1, iou=0.0, kind="touch", note="boxes that share an edge have inter = 0: kept at iou_thres = 0"),
    _nms("iou_neg", 300, 200, iou=-1.0, note="every later box is suppressed, disjoint and other-class ones included (ovr = 0 > -1)"),
    _nms("dups", 300, 200, jitter=0.0, entry="both", note="exact duplicates: IoU = 1"),
    _nms("zero_area", 300, 200, jitter=0.0, zero=0.5, note="duplicated zero-area boxes: 0 / 0 is not above any threshold"),
    _nms("ties", 600, 500, equal_scores=True, entry="both", note="one score for the whole candidate set: the order is the anchor index"),
    _nms("clsoff", 300, 240, nc=62, kind="clsoff", entry="both", note="the same box under classes 61, 60, 0: the offset keeps them apart"),
    _nms("rounding", 200, 96, B=1, nc=62, kind="rounding", note="48 pairs whose verdict hangs on fp32 rounding: 24 by the class offset, 24 by a contracted union"),
    _nms("max_nms", 32768, 32768, B=1, nc=2, kind="maxnms", survivors="==40", note="40 clusters; the 100 weakest candidates are isolated and ranked beyond NMS_MAX_NMS"),
]
NMS_N_EDGES = (0, 1, 2, 3, 255, 256, 257, 2047, 2048, 2049)
NMS_A_EDGES = (1, 1024, 1025, 16384, 16385)
NMS_REFUSED = [dict(id="max_det_4097", A=300, B=1, nc=4, max_det=NMS_MAX_DET + 1, text="bad shape"),
               dict(id="a_65537", A=NMS_MAX_A + 1, B=1, nc=1, max_det=300, text="exceeds 65536 anchors")]


def _dec(rid, levels, B, nc, kind="rand", dtypes=F16_F32, box_extra=0, cls_extra=0, straddle=(), optional=False, chain=False, note=""):
    """levels: ((h, w), ..) at strides 8, 16, 32.  box_extra / cls_extra: channels beyond 64 / beyond the padded class count, holding NaN.
    straddle: the seams ("image", "level1", "level2") that must fall inside a 64-anchor workgroup.  optional: also runs write_cls = 0 and no
    best-class outputs.  chain: cvmi_yolo_nms_best on the kernel's own best arrays."""
    A = sum(h * w for h, w in levels)
    return dict(id=rid, levels=tuple(levels), B=B, nc=nc, A=A, kind=kind, dtypes=dtypes, box_extra=box_extra, cls_extra=cls_extra, straddle=tuple(straddle),
                optional=optional, chain=chain, note=note)


def decode_tag(dt):
    return "detect_decode_kernel<%s>" % TNAME[dt]


def decode_seams(row):
    """{"image": [..], "level1": [..], "level2": [..]}: flat (image, anchor) indices at which a new image / level starts."""
    a0, out = 0, {"image": [b * row["A"] for b in range(1, row["B"])], "level1": [], "level2": []}
    for l, (h, w) in enumerate(row["levels"]):
        if l:
            out["level%d" % l] = [b * row["A"] + a0 for b in range(row["B"])]
        a0 += h * w
    return out


DECODE_NC_MAX = {"f16": 248, "f32": 252}          # 64 x (ncp + 1) floats in 64 KiB, ncp = nc rounded up to a 16-byte vector
DECODE_ROWS = [
    _dec("l3_seams", ((5, 7), (3, 4), (1, 1)), 3, 62, box_extra=16, cls_extra=16, straddle=("image", "level1", "level2"), optional=True,
         note="A = 48: workgroup 0 holds both level seams and the image seam; a 1 x 1 level; B * A = 144"),
    _dec("l1_64", ((8, 8),), 1, 8, note="B * A = 64: one full workgroup"),
    _dec("l1_1", ((1, 1),), 1, 1, note="B * A = 1, nc = 1"),
    _dec("l2_nonsquare", ((3, 9), (2, 5)), 2, 7, cls_extra=8, straddle=("image", "level1"), note="A = 37"),
    _dec("l3_nc80", ((6, 10), (3, 5), (2, 3)), 2, 80, box_extra=8, straddle=("image", "level2")),
    _dec("l3_ncmax_f16", ((3, 5), (2, 2), (1, 1)), 4, DECODE_NC_MAX["f16"], dtypes=("f16",), note="the widest class tile of the fp16 instance"),
    _dec("l3_ncmax_f32", ((3, 5), (2, 2), (1, 1)), 4, DECODE_NC_MAX["f32"], dtypes=("f32",)),
    _dec("cls_ties", ((4, 6), (2, 3)), 2, 62, kind="ties", straddle=("image", "level1"), note="equal logits in several channels: the first maximum wins"),
    _dec("saturated", ((4, 6), (2, 3)), 2, 7, kind="saturated", note="+-1000 in DFL bins and class logits"),
    _dec("chain", ((12, 20), (6, 10), (3, 5)), 2, 62, chain=True, straddle=("image", "level1", "level2"), note="decode -> cvmi_yolo_nms_best"),
]
DECODE_REFUSED = [dict(id="nc_249_f16", dt="f16", nc=DECODE_NC_MAX["f16"] + 1, text="nc too large"), dict(id="nc_253_f32", dt="f32", nc=DECODE_NC_MAX["f32"] + 1, text="nc too large"),
                  dict(id="score_without_cls", dt="f16", nc=8, best="score", text="go together"), dict(id="cls_without_score", dt="f32", nc=8, best="cls", text="go together")]

# mutant of tests/detect_ref.py -> ids of the rows whose expected output it must change (tests/test_detect_ref_cpu.py)
DETECT_MUTANT_ROWS = {
    "conf_ge": ["n0", "conf0", "lds_256_geo"],
    "iou_ge": ["iou0_touch"],
    "ties_desc_anchor": ["ties"],
    "no_class_offset": ["clsoff"],
    "area_unoffset": ["rounding"],
    "iou_fma": ["rounding"],
    "max_det_off_by_one": ["md1", "md300_more", "md4096_more"],
    "no_max_nms": ["max_nms"],
    "best_last_max": ["lds_256_geo", "cls_ties:decode"],
    "dfl_no_max": ["saturated:decode"],
    "anchor_no_half": ["l1_1:decode", "l3_seams:decode"],
    "level_seam_off_by_one": ["l3_seams:decode", "l2_nonsquare:decode"],
}
# mutants no row can see (none today): kept as a name so that a blind spot is recorded, never dropped
DETECT_UNSEEN_MUTANTS = {}


# ---- the resampling kernels: the five forms of cvmi_sam2_transform* and the bilinear mask return (resample.hip) -----------------------------------
# One transform row = a list of source images (H, W), a list of items (image, x0, y0, w, h) -- output b of the launch is that window of that
# image -- and the entry forms, output types and swap_rb values it runs through.  One mask-return row = one source shape and what it returns to.
# Operands, references, mutants and the bounds live in tests/resample_ref.py.  The constants below mirror resample.hip
# (tests/test_op_coverage_cpu.py holds them to the source text).
AA_MAXTAPS = 24                                    # taps per axis aa_axis keeps; the host guards refuse 2 * max(scale, 1) + 2 > AA_MAXTAPS
RECT_MAX = 64                                      # windows / rows / sizes per launch of the table-by-value entry points
AA_CAP_SCALE = (AA_MAXTAPS - 2) / 2                # 11: the largest legal down-scale
RESAMPLE_GRID_CAP = {"transform": 4096 * 256, "bilinear": 1024 * 256, "mask_extent": 32 * 256}      # work items of one grid pass
TRANSFORM_FORMS = ("single", "batch", "rects", "rects_dev", "srcs")
TRANSFORM_ENTRY = {"single": "cvmi_sam2_transform", "batch": "cvmi_sam2_transform_batch", "rects": "cvmi_sam2_transform_rects",
                   "rects_dev": "cvmi_sam2_transform_rects_dev", "srcs": "cvmi_sam2_transform_srcs"}
MASK_FORMS = ("bilinear_f32", "mask_postprocess", "mask_postprocess_sizes", "mask_postprocess_rects_dev", "mask_extent")
MASK_ENTRY = {f: "cvmi_" + f for f in MASK_FORMS}
MASK_THRESHOLDS = (0.0, 0.3, -1.5)
ALL_FORMS4 = ("batch", "rects", "rects_dev", "srcs")
WIN_FORMS = ("rects", "rects_dev", "srcs")


def _tf(rid, images, items=None, forms=ALL_FORMS4, dtypes=ALL3, swaps=(0, 1), R=16, stride0=False, fill="noise", refuse=None, tags=(), note=""):
    """items None: the whole of every image.  stride0: every item reads image 0 (`rects` / `rects_dev` with src_image_stride = 0).  fill "window":
    mid-grey noise inside each image's window and 0 / 255 outside it.  refuse: {form: text of the error}; the other forms of the row run."""
    images = [tuple(i) for i in images]
    if items is None:
        items = [(i, 0, 0, W, H) for i, (H, W) in enumerate(images)]
    return dict(op="transform", id="tf_" + rid, R=R, images=images, items=[tuple(i) for i in items], forms=tuple(forms), dtypes=tuple(dtypes), swaps=tuple(swaps),
                stride0=stride0, fill=fill, refuse=dict(refuse or {}), tags=tuple(tags), note=note)


def _mk(rid, hw, HW, N=2, forms=MASK_FORMS[:4], kind="blob", seed=0):
    return dict(op="mask", id="mask_" + rid, N=N, h=hw[0], w=hw[1], H=HW[0], W=HW[1], thresholds=MASK_THRESHOLDS, forms=tuple(forms), kind=kind, seed=seed)


TF_WIN_IMAGE = (40, 56)                            # H, W of the windowed rows' images
TF_WINDOWS = ((0, 0, 56, 40), (7, 5, 33, 21), (13, 17, 1, 1), (3, 9, 37, 1), (11, 2, 1, 29), (32, 20, 24, 20))   # whole, interior, 1 x 1, two strips, bottom-right
TF_CLIP_WINDOWS = ((-5, 3, 20, 10), (4, -7, 12, 20), (60, 5, 10, 10), (10, 10, 0, -3), (40, 8, 30, 12), (9, 31, 14, 25))   # x0 < 0, y0 < 0, x0 >= W, w <= 0, x0 + w > W, y0 + h > H


def _w65(b):
    x0, y0 = b % 5, b % 3
    return (b, x0, y0, 40 - x0 - b % 7, 24 - y0 - b % 4)


def _resample_rows():
    rows = [
        _tf("identity_16x16", [(16, 16)], forms=TRANSFORM_FORMS),
        _tf("up_1x1", [(1, 1)], forms=TRANSFORM_FORMS),
        _tf("up_2x3", [(2, 3)]),
        _tf("up_down_1x40", [(1, 40)], note="one axis up, one down"),
        _tf("down_24x40", [(24, 40)], forms=TRANSFORM_FORMS),
        _tf("down_37x53", [(37, 53)]),
        # ---- the cap: 2 * scale + 2 == AA_MAXTAPS at 176 source pixels
        _tf("cap_176x176", [(176, 176)], forms=TRANSFORM_FORMS, tags=("cap", "deep")),
        _tf("deep_175x131", [(175, 131)], swaps=(0,), tags=("deep",)),
        _tf("cap_176x5", [(176, 5)], swaps=(1,), tags=("cap", "deep"), note="the guard is per axis: 11 down, 3.2 up"),
        _tf("cap_window_176_in_200x300", [(200, 300)], [(0, 61, 13, 176, 176)], forms=("rects", "srcs"), fill="window", tags=("cap", "deep", "window"),
            note="rects_dev refuses this image: its guard is on the whole image"),
        # ---- refused: the output keeps its sentinel
        _tf("refuse_177x16", [(177, 16)], forms=TRANSFORM_FORMS, dtypes=("f32", "bf16"), swaps=(0,), tags=("refused",),
            refuse={"single": "sam2_transform: down-scale factor too large", "batch": "sam2_transform: down-scale factor too large",
                    "rects": "sam2_transform_rects: down-scale factor of window 0 too large",
                    "rects_dev": "sam2_transform_rects_dev: down-scale factor of the 16 x 177 image too large",
                    "srcs": "sam2_transform_srcs: down-scale factor of window 0 too large"}),
        _tf("refuse_16x177", [(16, 177)], forms=TRANSFORM_FORMS, dtypes=("f32", "f16"), swaps=(0,), tags=("refused",),
            refuse={"single": "sam2_transform: down-scale factor too large", "batch": "sam2_transform: down-scale factor too large",
                    "rects": "sam2_transform_rects: down-scale factor of window 0 too large",
                    "rects_dev": "sam2_transform_rects_dev: down-scale factor of the 177 x 16 image too large",
                    "srcs": "sam2_transform_srcs: down-scale factor of window 0 too large"}),
        _tf("refuse_window_177_high", [(180, 24)], [(0, 2, 1, 16, 177)], forms=("rects", "srcs"), dtypes=("f32", "f16"), swaps=(0,), tags=("refused",),
            refuse={"rects": "sam2_transform_rects: down-scale factor of window 0 too large", "srcs": "sam2_transform_srcs: down-scale factor of window 0 too large"}),
        _tf("small_window_in_177_high", [(177, 24)], [(0, 3, 4, 8, 8)], forms=WIN_FORMS, dtypes=("f32", "bf16"), swaps=(0,), fill="window", tags=("refused", "window"),
            refuse={"rects_dev": "sam2_transform_rects_dev: down-scale factor of the 24 x 177 image too large"},
            note="the documented whole-image guard of rects_dev; rects and srcs judge the window and run"),
        # ---- the second grid pass: R * R > 4096 * 256
        _tf("second_pass_8x8", [(8, 8)], R=1025, dtypes=("f32", "bf16"), swaps=(0,), tags=("second_pass",)),
        _tf("second_pass_40x24", [(40, 24)], R=1025, forms=("batch", "rects_dev"), dtypes=("f32", "f16"), swaps=(1,), tags=("second_pass",)),
        _tf("batch3", [(24, 40)] * 3),
        # ---- windows
        _tf("windows", [TF_WIN_IMAGE] * len(TF_WINDOWS), [(i,) + w for i, w in enumerate(TF_WINDOWS)], forms=WIN_FORMS, fill="window", tags=("window",)),
        _tf("windows_one_image", [TF_WIN_IMAGE], [(0,) + w for w in TF_WINDOWS], forms=WIN_FORMS, stride0=True, tags=("window",)),
        _tf("windows_65", [(24, 40)] * 65, [_w65(b) for b in range(65)], forms=("rects", "srcs"), swaps=(0,), fill="window", tags=("window", "second_table")),
        _tf("srcs_three_sizes", [(24, 40), (37, 53), (9, 11)], [(0, 3, 2, 30, 20), (1, 0, 0, 53, 37), (2, 4, 1, 5, 7), (1, 20, 9, 33, 28)], forms=("srcs",),
            fill="window", tags=("window",), note="item 3 reuses image 1: its outside pattern is image 1's window"),
        _tf("clip_rects_dev", [TF_WIN_IMAGE] * len(TF_CLIP_WINDOWS), [(i,) + w for i, w in enumerate(TF_CLIP_WINDOWS)], forms=("rects_dev",), tags=("clip",)),
        _tf("refuse_window_64_of_65", [(24, 40)] * 65, [_w65(b) if b < 64 else (64, 30, 2, 11, 10) for b in range(65)], forms=("rects", "srcs"), dtypes=("f32", "f16"),
            swaps=(0,), tags=("refused", "nothing_written"),
            refuse={"rects": "sam2_transform_rects: window 64 = (x 30, y 2, w 11, h 10) leaves the 40 x 24 image",
                    "srcs": "sam2_transform_srcs: window 64 = (x 30, y 2, w 11, h 10) leaves the 40 x 24 image"}),
        # ---- the mask return
        _mk("identity_9x7", (9, 7), (9, 7)),
        _mk("down_64_to_5x3", (64, 64), (5, 3)),
        _mk("down_64_to_1x1", (64, 64), (1, 1)),
        _mk("up_1x1_to_7x5", (1, 1), (7, 5)),
        _mk("up_2x2_to_7x5", (2, 2), (7, 5)),
        _mk("out_1x33", (12, 10), (1, 33)),
        _mk("out_33x1", (12, 10), (33, 1)),
        _mk("empty_and_full", (6, 5), (13, 11), kind="flat"),
        dict(op="mask_sizes", id="mask_sizes_65", N=65, h=12, w=10, sizes=[(1 + 3 * (n // 8), 1 + 4 * (n % 8)) for n in range(65)], thresholds=MASK_THRESHOLDS,
             forms=("mask_postprocess_sizes",), refuse=None, kind="edge", seed=0),
        dict(op="mask_sizes", id="mask_sizes_refuse_64_of_65", N=65, h=12, w=10, sizes=[(1 + 3 * (n // 8), 1 + 4 * (n % 8)) if n < 64 else (0, 5) for n in range(65)],
             thresholds=(0.0,), forms=("mask_postprocess_sizes",), refuse="mask_postprocess_sizes: plane 64 has size 0 x 5", seed=0),
        dict(op="mask_rects_dev", id="mask_rects_dev_clip", N=5, h=12, w=10, windows=[(3, 4, 40, 30), (0, 0, 1500, 3), (5, 5, 0, -2), (7, 7, 33, 30), (0, 0, 1000, 1)],
             plane_stride=1000, thresholds=MASK_THRESHOLDS, forms=("mask_postprocess_rects_dev",), kind="edge", seed=0),
        dict(op="mask_rects_dev", id="mask_rects_dev_513x512", N=1, h=64, w=64, windows=[(0, 0, 512, 513)], plane_stride=513 * 512, thresholds=MASK_THRESHOLDS,
             forms=("mask_postprocess_rects_dev",), seed=3),              # seed: moved until no value lies within the bound of a threshold
        dict(op="extent", id="extent_91x91", H=91, W=91, planes=[((0, 0), (90, 0), (0, 90), (90, 90)), ((58, 37),), ()], forms=("mask_extent",)),
    ]
    return rows


RESAMPLE_ROWS = _resample_rows()


def _tf_ids(pred):
    return [r["id"] for r in RESAMPLE_ROWS if r["op"] == "transform" and not (r["refuse"] and not set(r["forms"]) - set(r["refuse"])) and pred(r)]


# mutant of tests/resample_ref.py -> ids of the rows that must catch it (tests/test_resample_ref_cpu.py)
RESAMPLE_MUTANT_ROWS = {
    "aa_taps_capped_16": _tf_ids(lambda r: "deep" in r["tags"]),
    "aa_no_antialias": _tf_ids(lambda r: any(max(w, h) > r["R"] for _, _, _, w, h in r["items"])),
    "aa_center_no_half": _tf_ids(lambda r: any((w, h) != (1, 1) for _, _, _, w, h in r["items"])),
    "aa_window_reads_image": ["tf_cap_window_176_in_200x300", "tf_small_window_in_177_high", "tf_windows", "tf_windows_one_image", "tf_windows_65", "tf_srcs_three_sizes"],
    "aa_swap_moves_mean_std": _tf_ids(lambda r: 1 in r["swaps"]),
    "aa_second_window_table_restarts": ["tf_windows_65"],
    "bil_align_corners": ["mask_down_64_to_5x3", "mask_up_2x2_to_7x5", "mask_out_1x33", "mask_out_33x1", "mask_sizes_65", "mask_rects_dev_clip", "mask_rects_dev_513x512"],
    "bil_no_low_clamp": ["mask_up_2x2_to_7x5", "mask_out_1x33", "mask_out_33x1", "mask_sizes_65", "mask_rects_dev_clip"],   # the mask-only forms see it where a blob sits on the border
    "bil_extent_exclusive_max": ["mask_identity_9x7", "mask_down_64_to_5x3", "mask_up_2x2_to_7x5", "mask_empty_and_full", "mask_sizes_65", "mask_rects_dev_clip",
                                 "mask_rects_dev_513x512", "extent_91x91"],
    "clip_moves_window": ["tf_clip_rects_dev"],
}


# ---- the contour stage of wire_ops.hip: cvmi_external_contours and cvmi_node_prepare --------------------------------------------------------
# One CONTOUR row = one batch of planes (specs that tests/contour_ref.build_plane turns into arrays), whether the planes' sums are passed, and
# the tag cvmi_external_contours must leave in cvmi_last_kernel(): the trace path and its dynamic LDS bytes.  The constants mirror wire_ops.hip;
# tests/test_op_coverage_cpu.py compares them with the source text.
PLANE_MAX = 32                                     # planes per contour_table_kernel / node_empty_kernel launch
TRACE_LANES = 256                                  # contours traced per round of a plane's workgroup
ROOT_ROWS_PER_BLOCK = 4                            # one wave per row in root_count_kernel / root_assign_kernel
BALLOT_LANES = 64                                  # columns per ballot chunk of root_assign_kernel
CONTOUR_GRID_CAP = 1024 * 256                      # pixels one grid pass of the three label kernels (and of node_prepare's two) covers
TRACE_LDS_OPTIN = 64 * 1024                        # above: hipFuncSetAttribute(MaxDynamicSharedMemorySize)
TRACE_LDS_MAX = 160 * 1024                         # kLdsMax: above, the trace reads bytes from global memory


def plane_shape(spec):
    """(H, W) of a plane spec."""
    fixed = {"rings": (120, 160), "leak": (9, 11), "comb": (23, 61), "serpentine": (21, 37), "inv127": (15, 17), "inv127_plus1": (15, 17)}
    return fixed[spec[0]] if spec[0] in fixed else (spec[1], spec[2])


def trace_lds_bytes(shapes):
    """The bit planes of a batch in LDS: 4 bytes per 32 columns per row of the largest plane."""
    return 4 * max(h * ((w + 31) // 32) for h, w in shapes)


def contour_tag(shapes, lds_max=TRACE_LDS_MAX):
    """Mirror of cvmi_external_contours' choice, made once per batch from the largest plane."""
    lds = trace_lds_bytes(shapes)
    return "trace_kernel<lds, %d>" % lds if lds <= lds_max else "trace_kernel<global, 0>"


WORD_EDGE_W = (1, 31, 32, 33, 63, 64, 65, 129)
WORD_EDGE_H = (1, 4, 5, 9)
WORD_EDGE_PLANES = tuple(p for h in WORD_EDGE_H for w in WORD_EDGE_W for p in (("rand", h, w, 0.5, 1000 * h + w), ("full", h, w), ("lastrc", h, w)))


def _ct(rid, planes, expect, sums=True, note=""):
    return dict(id=rid, planes=tuple(planes), sums=sums, expect=expect, note=note)


def _lds_row(rid, tall, expect, note):
    return _ct(rid, WORD_EDGE_PLANES + (tall,), expect, sums=False, note=note)


CONTOUR_ROWS = [
    _ct("word_edges", WORD_EDGE_PLANES, "trace_kernel<lds, 180>", sums=False, note="the tail word, the frame rule, 64-wide ballot chunks, 4 rows per block"),
    _ct("lattice_9x129", [("lattice", 9, 129)], "trace_kernel<lds, 180>", sums=False, note="325 contours = the root capacity; the lane loop wraps; 65 roots per row"),
    _ct("nesting", [("rings",), ("leak",), ("comb", 23, 61), ("serpentine", 21, 37)], "trace_kernel<lds, 2400>", note="holes, the 4-connected background, revisited pixels"),
    _ct("inversion", [("inv127",), ("inv127_plus1",), ("values", 13, 19, 1, tuple(range(1, 101))), ("values", 13, 19, 2, tuple(range(150, 255))),
                      ("values", 16, 33, 3, (0, 0, 0, 7, 200, 255)), ("values", 16, 33, 4, (0, 7, 200, 255, 255, 255, 255))],
        "trace_kernel<lds, 128>", note="sum == 127 * H * W does not invert, + 1 does; both foreground rules; binarize"),
    _ct("inversion_no_sums", [("inv127_plus1",), ("values", 16, 33, 4, (0, 7, 200, 255, 255, 255, 255))], "trace_kernel<lds, 128>", sums=False,
        note="without sums nothing inverts"),
    _ct("empty_zero", [("zero", 7, 9), ("zero", 1, 1), ("zero", 40, 50)], "trace_kernel<lds, 320>", note="no contour: scan_kernel reads n = 0 from the device"),
    _ct("empty_full_inverts", [("full", 7, 9), ("full", 1, 1), ("full", 40, 50)], "trace_kernel<lds, 320>", note="all 255 inverts to nothing"),
    _ct("plane_max_plus_1", [("rand", 1 + (5 * n) % 8, 1 + (3 * n) % 8, 0.5, 50 + n) for n in range(PLANE_MAX)] + [("rand", 40, 50, 0.4, 99)], "trace_kernel<lds, 320>",
        note="the second contour_table_kernel launch with p0, r0, q0 carried"),
    _ct("grid_stride_513x512", [("rand", 513, 512, 0.35, 7)], "trace_kernel<lds, 32832>", sums=False, note="past the grid_for cap of the label kernels"),
    _lds_row("lds_64k_no_optin", ("stripes", 16384, 1, 0), "trace_kernel<lds, 65536>", "the largest request without the opt-in"),
    _lds_row("lds_64k_plus_optin", ("stripes", 16385, 1, 0), "trace_kernel<lds, 65540>", "the smallest request with the opt-in"),
    _lds_row("lds_160k_exact", ("stripes", 40960, 1, 0), "trace_kernel<lds, 163840>", "exactly kLdsMax"),
    _lds_row("global_160k_plus", ("stripes", 40961, 1, 0), "trace_kernel<global, 0>", "one row past kLdsMax: bytes from global memory"),
    _lds_row("global_40961x2", ("stripes", 40961, 2, 1), "trace_kernel<global, 0>", "the global path with a ragged last column"),
]
CONTOUR_CAPACITY_ROW = _ct("capacity_lattice_rings", [("lattice", 9, 129), ("rings",)], "trace_kernel<lds, 2400>", sums=False, note="the capacity cases")
CONTOUR_CAPACITY_CASES = ("exact", "contours_minus_1", "points_minus_1", "count_only")


# One PREPARE row = the planes (H, W, seed) of one prepare_packed(new_height = PREPARE_HEIGHT) call and the boxes of each plane: "kinds" = the
# box kinds of tests/test_wires_gpu.py (negative, past the edge, empty, preserved, a fractional one), "none" = no box.
PREPARE_HEIGHT = 12
PREPARE_REFUSED = ((40, 1),)                       # int(12 * (1 / 40)) = 0 columns: prepare_packed refuses what cv2.resize would reject


def _pp(rid, planes, boxes, note=""):
    return dict(id=rid, planes=tuple(planes), boxes=tuple(boxes), note=note)


PREPARE_ROWS = [
    _pp("identity_12x18", [(12, 18, 1)], ["kinds"], "NH == H and NW == W: the copy branch"),
    _pp("down_2x_24x36", [(24, 36, 2)], ["kinds"], "an exact 2x downscale"),
    _pp("up_from_5x7", [(5, 7, 3)], ["kinds"], "an upscale"),
    _pp("ratio_37x53", [(37, 53, 4)], ["kinds"], "a non-integer ratio"),
    _pp("tiny_1x1_1x40", [(1, 1, 5), (1, 40, 6)], ["kinds", "kinds"], "one-pixel axes"),
    _pp("thin_2x300", [(2, 300, 7)], ["kinds"], "a thin plane"),
    _pp("grid_stride_513x512", [(513, 512, 8)], ["kinds"], "past the grid cap of node_empty_kernel"),
    _pp("plane_max_plus_1", [(3 + n % 5, 4 + n % 7, 20 + n) for n in range(PLANE_MAX + 1)], ["none"] * (PLANE_MAX - 1) + ["kinds", "kinds"],
        "boxes only on the last plane of the first launch and the only plane of the second: box0 of the second launch"),
    _pp("mixed_no_box", [(12, 18, 9), (9, 14, 10), (24, 36, 11)], ["kinds", "none", "kinds"], "a plane with no box between two that have them"),
]
