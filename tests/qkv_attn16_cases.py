"""The table of the fused qkv + 4 x 4-window attention launch (csrc/qkv_attn16.hpp), shared by tests/test_qkv_attn16_gpu.py and its CPU guard.

A row: id, the grid (B, H, W) of tokens, the block's (K, heads, q_pool) and the kernel tag cvmi_last_kernel() must report.  Every grid has H, W
multiples of 4 and B * H * W a multiple of 256 (the unfused oracle takes 256-row workgroups; the fused launch 128 tokens = eight windows).
Grids: 256 tokens, the smallest (two workgroups); six windows per grid row (no power of two), 768 tokens; two window rows of eight; one window
per grid row over four images.  The q-pooled rows (K = 288 -> 576, 8 heads, 4 queries per window and head, `ao` on the half-resolution grid) run
the first two."""

QKV_ATTN16_ROWS = [
    dict(id="plain_1x16x16", grid=(1, 16, 16), K=288, heads=4, q_pool=0, expect="qkv_attn16_kernel<288, 4, false>"),
    dict(id="plain_2x16x24", grid=(2, 16, 24), K=288, heads=4, q_pool=0, expect="qkv_attn16_kernel<288, 4, false>"),
    dict(id="plain_1x8x32", grid=(1, 8, 32), K=288, heads=4, q_pool=0, expect="qkv_attn16_kernel<288, 4, false>"),
    dict(id="plain_4x64x4", grid=(4, 64, 4), K=288, heads=4, q_pool=0, expect="qkv_attn16_kernel<288, 4, false>"),
    dict(id="qpool_1x16x16", grid=(1, 16, 16), K=288, heads=8, q_pool=1, expect="qkv_attn16_kernel<288, 8, true>"),
    dict(id="qpool_2x16x24", grid=(2, 16, 24), K=288, heads=8, q_pool=1, expect="qkv_attn16_kernel<288, 8, true>"),
    # kinds=1: the leading token rows carry the five LayerNorm row kinds of tests/tok_ref.py row_kinds, one per instance
    dict(id="kinds_2x16x24", grid=(2, 16, 24), K=288, heads=4, q_pool=0, kinds=1, expect="qkv_attn16_kernel<288, 4, false>"),
    dict(id="kinds_qpool_2x16x24", grid=(2, 16, 24), K=288, heads=8, q_pool=1, kinds=1, expect="qkv_attn16_kernel<288, 8, true>"),
]
