"""The table of the fused qkv + window-attention launch (csrc/qkv_attn.hpp), shared by tests/test_qkv_attn_gpu.py and its CPU guard.

A row: id, the grid (B, H, W) of tokens, the block's (K, heads, q_pool) and the kernel tag cvmi_last_kernel() must report.  Grids: one or two
workgroups; three windows per grid row (no power of two), 768 tokens; one window row of four; twelve windows in a single column over three
images.  The q-pooled rows (K = 144 -> 288, 4 heads, 16 queries per window and head, `ao` on the half-resolution grid) run the first two."""

QKV_ATTN_ROWS = [
    dict(id="plain_1x16x16", grid=(1, 16, 16), K=144, heads=2, q_pool=0, expect="qkv_attn64_kernel<144, 2, false>"),
    dict(id="plain_2x16x24", grid=(2, 16, 24), K=144, heads=2, q_pool=0, expect="qkv_attn64_kernel<144, 2, false>"),
    dict(id="plain_1x8x32", grid=(1, 8, 32), K=144, heads=2, q_pool=0, expect="qkv_attn64_kernel<144, 2, false>"),
    dict(id="plain_3x32x8", grid=(3, 32, 8), K=144, heads=2, q_pool=0, expect="qkv_attn64_kernel<144, 2, false>"),
    dict(id="qpool_1x16x16", grid=(1, 16, 16), K=144, heads=4, q_pool=1, expect="qkv_attn64_kernel<144, 4, true>"),
    dict(id="qpool_2x16x24", grid=(2, 16, 24), K=144, heads=4, q_pool=1, expect="qkv_attn64_kernel<144, 4, true>"),
    # kinds=1: the leading token rows carry the five LayerNorm row kinds of tests/tok_ref.py row_kinds, one per instance
    dict(id="kinds_2x16x24", grid=(2, 16, 24), K=144, heads=2, q_pool=0, kinds=1, expect="qkv_attn64_kernel<144, 2, false>"),
    dict(id="kinds_qpool_2x16x24", grid=(2, 16, 24), K=144, heads=4, q_pool=1, kinds=1, expect="qkv_attn64_kernel<144, 4, true>"),
]
