"""Case tables shared by the per-op GPU suites and the CPU coverage guard (tests/test_op_coverage_cpu.py).

ATTN_ROWS: the attention dispatch matrix.  One row = one shape and layout of cvmi_attention and the kernel that cvmi_last_kernel() must name
after the launch (attention.hip, cvmi_attention: the dispatcher with default settings).  Kernel names do not carry the operand type, so one
expected name serves fp16 and bf16.

BF16_OPS: every entry point that common.hpp builds twice (CVMI_ENTRY) -> (test module, test function) that checks its bf16 build per op.

Plain data: importing this module needs neither a GPU nor the library."""

F16_BF16 = ("f16", "bf16")


def _row(rid, expect, B, heads, Nq, Nk, dqk, dv, dtypes=F16_BF16, layout="sep", o_pad=0, q_log2=0, note=""):
    """Global (non-window) attention.  layout: "sep" = q, k, v in three [B, N, heads * d] buffers; "qkv" = one fused [B, N, (2 dqk + dv) heads]
    buffer (needs Nq == Nk); "kv256" = the decoder's K and V halves of one [B, Nk, heads * (dqk + dv)] buffer.  o_pad > 0: the output sits at
    column o_pad of a buffer o_pad columns wider on both sides."""
    return dict(id=rid, expect=expect, B=B, heads=heads, Nq=Nq, Nk=Nk, dqk=dqk, dv=dv, dtypes=dtypes, layout=layout, o_pad=o_pad,
                q_log2=q_log2, win=0, note=note)


def _win(rid, expect, imgs, gh, gw, heads, win, q_pool=0, dtypes=F16_BF16, o_pad=0, q_log2=0, note=""):
    """Hiera window attention straight off a fused NHWC [imgs, gh, gw, 3 C] q/k/v grid (k_st = 3 C), head_dim 72, optional 2 x 2 q max-pool."""
    nwin = imgs * (gh // win) * (gw // win)
    Nq = (win // 2) ** 2 if q_pool else win * win
    return dict(id=rid, expect=expect, B=nwin, heads=heads, Nq=Nq, Nk=win * win, dqk=72, dv=72, dtypes=dtypes, layout="grid", o_pad=o_pad,
                q_log2=q_log2, win=win, imgs=imgs, gh=gh, gw=gw, q_pool=q_pool, note=note)


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

# dual-built entry point -> (test module, test function) that checks its bf16 build op by op
BF16_OPS = {
    "cvmi_attention": ("test_attention_matrix_gpu.py", "test_attention_matrix"),
    "cvmi_conv2d": ("test_bf16_ops_gpu.py", "test_conv2d_bf16"),
    "cvmi_layernorm": ("test_bf16_ops_gpu.py", "test_layernorm_bf16"),
    "cvmi_layernorm_dual": ("test_bf16_ops_gpu.py", "test_layernorm_dual_bf16_copy"),
    "cvmi_maxpool2x2": ("test_bf16_ops_gpu.py", "test_maxpool_and_space_to_depth_bf16"),
    "cvmi_space_to_depth4": ("test_bf16_ops_gpu.py", "test_maxpool_and_space_to_depth_bf16"),
    "cvmi_cast": ("test_bf16_ops_gpu.py", "test_cast_bf16"),
    "cvmi_nchw_to_nhwc": ("test_bf16_ops_gpu.py", "test_nchw_to_nhwc_bf16"),
    "cvmi_prompt_tokens": ("test_bf16_ops_gpu.py", "test_prompt_tokens_bf16"),
    "cvmi_hyper_masks": ("test_bf16_ops_gpu.py", "test_hyper_masks_bf16"),
    "cvmi_sam2_transform_batch": ("test_crop_gpu.py", "test_transform_from_windows_is_bit_identical_to_transforming_crops"),
    "cvmi_sam2_transform_rects": ("test_crop_gpu.py", "test_transform_from_windows_is_bit_identical_to_transforming_crops"),
    "cvmi_hiera_mlp": ("test_ops_gpu.py", "test_hiera_mlp_fused_vs_torch"),
    "cvmi_hiera_mlp_stats": ("test_ops_gpu.py", "test_hiera_mlp_fused_vs_torch"),
    "cvmi_tok_linear": ("test_ops_gpu.py", "test_tok_linear_vs_torch"),
    "cvmi_tok_linear_stats": ("test_ops_gpu.py", "test_tok_linear_forwarded_layernorm_statistics"),
    "cvmi_tok_linear_pool": ("test_ops_gpu.py", "test_tok_linear_pool_vs_torch"),
    "cvmi_tok_linear_pool_stats": ("test_ops_gpu.py", "test_tok_linear_pool_vs_torch"),
    "cvmi_tok_linear16_launch": ("test_ops_gpu.py", "test_tok_linear16_row_blocks_shared_between_workgroups"),
    "cvmi_tok_linear16_splits": ("test_ops_gpu.py", "test_tok_linear16_row_blocks_shared_between_workgroups"),
}
