"""CPU guard of the fused qkv + window-attention launch (csrc/qkv_attn.hpp): what the descriptor refuses, that every instance the header can
launch has a row in tests/qkv_attn_cases.py, and that the packed row permutation gives back W and b."""
import ctypes
import os
import re

import pytest
import torch

from circuitvision_amd import _lib
from circuitvision_amd._lib import BF16, F16, F32
from circuitvision_amd.engine import TORCH_DTYPE, PackedQkvAttn, make_attn_desc, qkv_attn_rows, qkv_attn_supported
from qkv_attn_cases import QKV_ATTN_ROWS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "circuitvision_amd", "csrc", "qkv_attn.hpp")
needs_lib = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="libcvmi355.so not built")


def header_instances(text):
    """Tags of every instance the header's dispatcher can launch, spelled as its cvmi_note_kernel format spells them."""
    return ["qkv_attn64_kernel<%s, %s, %s>" % m for m in re.findall(r"return launch_qkv_attn<(\d+), (\d+), (true|false)>\(", text)]


def test_every_instance_the_header_launches_has_a_row():
    text = open(HEADER).read()
    # the tag: the shared launcher (qa_launch) formats its caller's format string with (K, heads, q-pooled)
    assert 'cvmi_note_kernel(tag, K, heads, CVMI_BOOLNAME(qpool));' in text
    assert re.findall(r'return qa_launch<&(\w+)<K, HEADS, QPOOL>, [^(]*\("([^"]*)", K, HEADS, QPOOL, a, ps, stream\);', text) == [("qkv_attn64_kernel", "qkv_attn64_kernel<%d, %d, %s>")]
    inst = header_instances(text)
    assert inst and len(inst) == len(set(inst)), inst       # the parser still finds the call sites
    tags = {r["expect"] for r in QKV_ATTN_ROWS}
    assert set(inst) == tags, (inst, tags)
    probe = text + "\n  return launch_qkv_attn<144, 8, true>(a, ps, stream);\n"
    assert set(header_instances(probe)) - tags == {"qkv_attn64_kernel<144, 8, true>"}
    for r in QKV_ATTN_ROWS:
        B, H, W = r["grid"]
        assert H % 8 == 0 and W % 8 == 0 and (B * H * W) % 256 == 0, r["id"]       # whole windows; the unfused oracle takes 256-row workgroups
        assert qkv_attn_supported(r["K"], r["heads"] * 72, r["heads"], 8, r["q_pool"], F16, B * H * W // 64), r["id"]
    assert any((r["grid"][2] // 8) & (r["grid"][2] // 8 - 1) for r in QKV_ATTN_ROWS), "no row whose windows per grid row are no power of two"


def test_the_plan_predicate_names_the_built_shapes():
    ok = lambda **kw: qkv_attn_supported(**{**dict(dim=144, dout=144, heads=2, ws=8, q_pool=False, dtype=F16, nwin=1024), **kw})
    assert ok() and ok(dtype=BF16) and ok(dout=288, heads=4, q_pool=True)
    assert not ok(dtype=F32) and not ok(dim=288, dout=288, heads=4) and not ok(dim=288, dout=576, heads=8, q_pool=True) and not ok(ws=4) and not ok(ws=16)
    assert not ok(ws=0) and not ok(q_pool=True) and not ok(nwin=3) and not ok(heads=4) and not ok(dout=288, heads=4) and not ok(dout=288, heads=2, q_pool=True)


@needs_lib
def test_the_descriptor_refuses_every_unsupported_combination():
    """Each refusal happens on the host before anything is launched (no GPU needed); the pointers are never dereferenced."""
    lib = _lib.load()
    A = 1 << 20                                              # an aligned, never-dereferenced address
    good = dict(q=None, k=None, v=None, o=A, q_sb=0, q_sh=72, q_st=432, k_sb=0, k_sh=72, k_st=432, v_sb=0, v_sh=72, v_st=432, o_sb=0, o_sh=72, o_st=144,
                B=4, heads=2, Nq=64, Nk=64, dqk=72, dv=72, scale=72 ** -0.5, dtype=F16, win=8, grid_h=16, grid_w=16, q_pool=0, q_bdiv=0, kv_bdiv=0,
                av_fp8=0, q_log2=0, proj_x=A, proj_w=A, proj_gamma=A, proj_beta=A, proj_stats=None, proj_ld=144, proj_K=144, proj_eps=1e-6)

    def refused(match, **kw):
        d = make_attn_desc(**{**good, **kw})
        rc = lib.cvmi_attention(ctypes.byref(d), None)
        assert rc != 0, kw
        with pytest.raises(_lib.CvmiError, match=match):
            _lib.check(rc, "qkv_attn")

    for dtype in (F16, BF16):
        refused("16-bit dtype", dtype=F32)
        refused("8 x 8 windows of head_dim 72", dtype=dtype, win=16, Nq=256, Nk=256)
        refused("8 x 8 windows of head_dim 72", dtype=dtype, win=4, Nq=16, Nk=16, grid_h=16, grid_w=16, B=16)
        refused("8 x 8 windows of head_dim 72", dtype=dtype, dqk=64, dv=64)
        refused("K=288 is not built", dtype=dtype, proj_K=288, proj_ld=288, heads=4)
        refused("heads=2 is not built", dtype=dtype, q_pool=1, Nq=16)
        refused("heads=4 is not built", dtype=dtype, heads=4)
        refused("heads=8 is not built", dtype=dtype, heads=8, q_pool=1, Nq=16)
        refused("no whole number of 128-token workgroups", dtype=dtype, B=3, grid_h=8, grid_w=24)
        refused("needs the packed weight", dtype=dtype, proj_w=None)
        refused("needs the packed weight", dtype=dtype, proj_gamma=None)
        refused("not aligned", dtype=dtype, proj_ld=140)
        refused("not aligned", dtype=dtype, proj_ld=146)
        refused("not aligned", dtype=dtype, proj_x=A + 4)
        refused("not aligned", dtype=dtype, proj_stats=A + 4)
        refused("output strides", dtype=dtype, o_st=146)
        refused("8 x 8 windows of head_dim 72", dtype=dtype, win=0, grid_h=0, grid_w=0)
    refused("null pointer", proj_x=None)                      # no projection source and no q / k / v
    assert lib.cvmi_version() >= 126                          # 126: cvmi_attn_desc.proj_*


@needs_lib
@pytest.mark.parametrize("heads", [2, 4])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_packed_permutation_round_trips(dtype, heads):
    hd, K = 72, 144
    N = 3 * heads * hd
    rows = qkv_attn_rows(heads, hd)
    assert len(rows) == heads * 256 and sorted(r for r in rows if r >= 0) == list(range(N))      # every row of W exactly once
    g = torch.Generator().manual_seed(5)
    w, b = torch.randn(N, K, generator=g), torch.randn(N, generator=g)
    pq = PackedQkvAttn(w, b, heads, "cpu", dtype)
    assert pq.rows == rows and pq.w.numel() * 2 == heads * 8 * (K // 16 + 1) * 1024
    wx = pq.w.float().view(heads * 8, K // 16 + 1, 2, 32, 8).permute(0, 3, 1, 2, 4).reshape(heads * 256, K + 16)      # (j, s, h, r, e) -> [row, k]
    td = TORCH_DTYPE[dtype]
    w_back, b_back = torch.zeros(N, K), torch.zeros(N)
    for i, r in enumerate(rows):
        if r < 0:
            assert not wx[i].any(), f"padding row {i} is not zero"
        else:
            w_back[r], b_back[r] = wx[i, :K], wx[i, K] + wx[i, K + 1]
            assert not wx[i, K + 2:].any()
    assert torch.equal(w_back, w.to(td).float())
    b_hi = b.to(td).float()
    assert torch.equal(b_back, b_hi + (b - b_hi).to(td).float())
    # the q chunks' order: chunk row 8 g + 4 lh + e of chunk c holds q channel 32 c + 16 (g >> 1) + 8 lh + 4 (g & 1) + e
    for h in range(heads):
        for c in range(3):
            for s2 in range(2):
                for lh in range(2):
                    frag = [rows[h * 256 + 32 * c + 8 * (2 * s2 + (i >> 2)) + 4 * lh + (i & 3)] for i in range(8)]
                    d0 = 32 * c + 16 * s2 + 8 * lh
                    assert frag == [h * hd + d0 + i if d0 + i < hd else -1 for i in range(8)], (h, c, s2, lh)
