#!/usr/bin/env python3
"""A/B of two builds of libcvmi355.so on the fused qkv + window attention launches, one build per process (CVMI_LIB_PATH selects it):
profiles/qkv_attn_refactor_ab.md.

Every row of QKV_ATTN_ROWS and QKV_ATTN16_ROWS in fp16 and bf16, q_log2 0 and 1, LayerNorm statistics absent and forwarded, on the operands of
tests/test_qkv_attn_gpu.py / tests/test_qkv_attn16_gpu.py (their generators, seeds and NaN padding): one line
"window row dtype q_log2 stats tag sha256(whole ao buffer, guard columns included)".  The tests assert that these kernels replay bit-identically,
so two builds compute the same thing iff their outputs are equal as text.
"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

from circuitvision_amd import _lib  # noqa: E402
from circuitvision_amd._lib import BF16, F16, F32  # noqa: E402
from circuitvision_amd.engine import TORCH_DTYPE, PackedQkvAttn, Plan, Rows, make_attn_desc, op_attention  # noqa: E402

from test_attention_matrix_gpu import LOG2E, SENTINEL  # noqa: E402

HD, PADR, OPAD, EPS = 72, 8, 8, 1e-6


def launch_hashes(lib, row, win, seed_mul, w_std, dt, dtype, q_log2):
    td = TORCH_DTYPE[dtype]
    (B, H, W), K, heads, qp = row["grid"], row["K"], row["heads"], row["q_pool"]
    C_, rows, ld = heads * HD, B * H * W, K + 4
    nwin = rows // (win * win)
    orows, nq = (rows // 4, win * win // 4) if qp else (rows, win * win)
    g = torch.Generator().manual_seed(seed_mul * rows + K + q_log2)
    w = torch.randn(3 * C_, K, generator=g) * w_std
    bias = torch.randn(3 * C_, generator=g) * 0.1
    if q_log2:
        w[:C_] *= HD ** -0.5 * LOG2E
        bias[:C_] *= HD ** -0.5 * LOG2E
    gam, bet = (1 + 0.2 * torch.randn(K, generator=g)).cuda(), (0.1 * torch.randn(K, generator=g)).cuda()
    xh = torch.randn(rows, K, generator=g) * (1 + torch.rand(rows, 1, generator=g)) + torch.randn(rows, 1, generator=g)
    xbuf = torch.full((PADR + rows, ld), float("nan"))
    xbuf[PADR:, :K] = xh
    xbuf = xbuf.cuda()
    x_rows = Rows(xbuf, rows, K, ld=ld, offset=PADR * ld, dtype=F32)
    mean = xh.mean(1)
    own = torch.stack((mean, 1.0 / torch.sqrt(((xh - mean[:, None]) ** 2).mean(1) + EPS)), 1).contiguous().cuda()
    pq = PackedQkvAttn(w, bias, heads, "cuda", dtype)
    for stats in (None, own):
        o = torch.full((orows, C_ + 2 * OPAD), SENTINEL, dtype=td, device="cuda")
        desc = make_attn_desc(q=None, k=None, v=None, o=o.data_ptr() + OPAD * o.element_size(), q_sb=0, q_sh=HD, q_st=3 * C_, k_sb=0, k_sh=HD, k_st=3 * C_,
                              v_sb=0, v_sh=HD, v_st=3 * C_, o_sb=0, o_sh=HD, o_st=C_ + 2 * OPAD, B=nwin, heads=heads, Nq=nq, Nk=win * win, dqk=HD, dv=HD,
                              scale=123.0 if q_log2 else HD ** -0.5, dtype=dtype, win=win, grid_h=H, grid_w=W, q_pool=qp, q_bdiv=0, kv_bdiv=0, av_fp8=0,
                              q_log2=q_log2, proj_x=x_rows.ptr, proj_ld=ld, proj_K=K, proj_w=pq.w.data_ptr(), proj_gamma=gam.data_ptr(),
                              proj_beta=bet.data_ptr(), proj_eps=EPS, proj_stats=stats.data_ptr() if stats is not None else None)
        plan = Plan(torch.cuda.Stream())
        op_attention(plan, "qkv_attn", desc, (xbuf, o, pq, gam, bet, stats))
        lib.cvmi_last_kernel()
        torch.cuda.synchronize()
        plan.run_eager()
        plan.stream.synchronize()
        tag = lib.cvmi_last_kernel().decode()
        assert tag == row["expect"], (tag, row["expect"])
        h = hashlib.sha256(o.cpu().view(torch.uint8).numpy().tobytes()).hexdigest()
        print(f"{win}x{win} {row['id']} {dt} q_log2={q_log2} stats={'absent' if stats is None else 'forwarded'} {tag} {h}", flush=True)


def main():
    from qkv_attn16_cases import QKV_ATTN16_ROWS
    from qkv_attn_cases import QKV_ATTN_ROWS
    lib = _lib.load()
    for table, win, seed_mul, w_std in ((QKV_ATTN_ROWS, 8, 17, 0.08), (QKV_ATTN16_ROWS, 4, 19, 0.06)):      # (the two tests' seeds and weight scales)
        for row in table:
            for dt, dtype in (("f16", F16), ("bf16", BF16)):
                for q_log2 in (0, 1):
                    launch_hashes(lib, row, win, seed_mul, w_std, dt, dtype, q_log2)


if __name__ == "__main__":
    main()
