"""CPU guard of the fused qkv + 4 x 4-window attention launch (csrc/qkv_attn16.hpp): what the descriptor refuses, that every instance the
header can launch has a row in tests/qkv_attn16_cases.py (and every row an instance), that the plan's predicate names exactly the built
shapes, and that the packed row permutation gives back W and b for both head counts."""
import ctypes
import os
import re

import pytest
import torch

from circuitvision_amd import _lib
from circuitvision_amd._lib import BF16, F16, F32
from circuitvision_amd.engine import TORCH_DTYPE, PackedQkvAttn, make_attn_desc, qkv_attn16_supported, qkv_attn_rows, qkv_attn_supported
from qkv_attn16_cases import QKV_ATTN16_ROWS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "circuitvision_amd", "csrc", "qkv_attn16.hpp")
needs_lib = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="libcvmi355.so not built")


def header_instances(text):
    """Tags of every instance the header's dispatcher can launch, spelled as its cvmi_note_kernel format spells them."""
    return ["qkv_attn16_kernel<%s, %s, %s>" % m for m in re.findall(r"return launch_qkv_attn16<(\d+), (\d+), (true|false)>\(", text)]


def test_every_instance_the_header_launches_has_a_row_and_every_row_an_instance():
    text = open(HEADER).read()
    # the tag: the shared launcher (qa_launch of qkv_attn.hpp) formats its caller's format string with (K, heads, q-pooled)
    assert 'cvmi_note_kernel(tag, K, heads, CVMI_BOOLNAME(qpool));' in open(os.path.join(os.path.dirname(HEADER), "qkv_attn.hpp")).read()
    assert re.findall(r'return qa_launch<&(\w+)<K, HEADS, QPOOL>, [^(]*\("([^"]*)", K, HEADS, QPOOL, a, ps, stream\);', text) == [("qkv_attn16_kernel", "qkv_attn16_kernel<%d, %d, %s>")]
    inst = header_instances(text)
    assert inst and len(inst) == len(set(inst)), inst       # the parser still finds the call sites
    tags = {r["expect"] for r in QKV_ATTN16_ROWS}
    assert set(inst) == tags, (inst, tags)
    probe = text + "\n  return launch_qkv_attn16<288, 2, true>(a, ps, stream);\n"
    assert set(header_instances(probe)) - tags == {"qkv_attn16_kernel<288, 2, true>"}
    ids = [r["id"] for r in QKV_ATTN16_ROWS]
    assert len(ids) == len(set(ids))
    for r in QKV_ATTN16_ROWS:
        B, H, W = r["grid"]
        assert H % 4 == 0 and W % 4 == 0 and (B * H * W) % 256 == 0, r["id"]       # whole windows; the unfused oracle takes 256-row workgroups
        assert r["expect"] == "qkv_attn16_kernel<%d, %d, %s>" % (r["K"], r["heads"], "true" if r["q_pool"] else "false"), r["id"]
        assert qkv_attn16_supported(r["K"], r["heads"] * 72, r["heads"], 4, r["q_pool"], F16, B * H * W // 16), r["id"]
    assert any((r["grid"][2] // 4) & (r["grid"][2] // 4 - 1) for r in QKV_ATTN16_ROWS), "no row whose windows per grid row are no power of two"
    assert any(r["grid"][2] == 4 and r["grid"][0] > 1 for r in QKV_ATTN16_ROWS), "no row with one window per grid row over several images"
    assert "getenv" not in text                              # dispatch depends on shapes alone


def test_the_plan_predicate_names_the_built_shapes():
    ok = lambda **kw: qkv_attn16_supported(**{**dict(dim=288, dout=288, heads=4, ws=4, q_pool=False, dtype=F16, nwin=1024), **kw})
    assert ok() and ok(dtype=BF16) and ok(dout=576, heads=8, q_pool=True) and ok(nwin=8)
    assert not ok(dtype=F32) and not ok(dim=144, dout=144, heads=2) and not ok(dim=576, dout=576, heads=8) and not ok(ws=8) and not ok(ws=16) and not ok(ws=0)
    assert not ok(q_pool=True) and not ok(nwin=4) and not ok(nwin=12) and not ok(heads=2) and not ok(heads=8) and not ok(dout=576, heads=8)
    assert not ok(dout=576, heads=4, q_pool=True)
    # the two predicates never claim the same block
    for dim, dout, heads, ws, qp in ((144, 144, 2, 8, False), (144, 288, 4, 8, True), (288, 288, 4, 4, False), (288, 576, 8, 4, True)):
        assert qkv_attn_supported(dim, dout, heads, ws, qp, F16, 1024) != qkv_attn16_supported(dim, dout, heads, ws, qp, F16, 1024)


@needs_lib
def test_the_descriptor_refuses_every_unsupported_combination():
    """Each refusal happens on the host before anything is launched (no GPU needed); the pointers are never dereferenced."""
    lib = _lib.load()
    A = 1 << 20                                              # an aligned, never-dereferenced address
    good = dict(q=None, k=None, v=None, o=A, q_sb=0, q_sh=72, q_st=864, k_sb=0, k_sh=72, k_st=864, v_sb=0, v_sh=72, v_st=864, o_sb=0, o_sh=72, o_st=288,
                B=16, heads=4, Nq=16, Nk=16, dqk=72, dv=72, scale=72 ** -0.5, dtype=F16, win=4, grid_h=16, grid_w=16, q_pool=0, q_bdiv=0, kv_bdiv=0,
                av_fp8=0, q_log2=0, proj_x=A, proj_w=A, proj_gamma=A, proj_beta=A, proj_stats=None, proj_ld=288, proj_K=288, proj_eps=1e-6)

    def refused(match, **kw):
        d = make_attn_desc(**{**good, **kw})
        rc = lib.cvmi_attention(ctypes.byref(d), None)
        assert rc != 0, kw
        with pytest.raises(_lib.CvmiError, match=match):
            _lib.check(rc, "qkv_attn16")

    for dtype in (F16, BF16):
        refused("16-bit dtype", dtype=F32)
        refused("4 x 4 windows of head_dim 72", dtype=dtype, dqk=64, dv=64)
        refused("4 x 4 windows of head_dim 72", dtype=dtype, dv=64)
        refused("Nk == win\\^2", dtype=dtype, Nk=64, Nq=64)   # (window mode's own check: no 4 x 4 request carries another key count)
        refused("heads=2 is not built", dtype=dtype, heads=2)
        refused("heads=8 is not built", dtype=dtype, heads=8)
        refused("heads=4 is not built", dtype=dtype, q_pool=1, Nq=4)
        refused("heads=16 is not built", dtype=dtype, heads=16, q_pool=1, Nq=4)
        refused("no whole number of 128-token workgroups", dtype=dtype, B=4, grid_h=8, grid_w=8)
        refused("no whole number of 128-token workgroups", dtype=dtype, B=12, grid_h=8, grid_w=24)
        refused("batch sharing", dtype=dtype, q_bdiv=2)
        refused("batch sharing", dtype=dtype, kv_bdiv=2)
        refused("needs the packed weight", dtype=dtype, proj_w=None)
        refused("needs the packed weight", dtype=dtype, proj_beta=None)
        refused("not aligned", dtype=dtype, proj_ld=284)
        refused("not aligned", dtype=dtype, proj_ld=290)
        refused("not aligned", dtype=dtype, proj_x=A + 4)
        refused("not aligned", dtype=dtype, proj_w=A + 8)
        refused("not aligned", dtype=dtype, proj_stats=A + 4)
        refused("output strides", dtype=dtype, o_st=290)
        refused("output strides", dtype=dtype, o_sh=74)
        refused("output strides", dtype=dtype, o=A + 4)
        refused("no fp8 AV product", dtype=dtype, av_fp8=1)
        # the neighbouring shapes stay with the 8 x 8 header's dispatcher and its refusals
        refused("8 x 8 windows of head_dim 72", dtype=dtype, proj_K=144, proj_ld=144)
        refused("K=288 is not built", dtype=dtype, win=8, Nq=64, Nk=64, B=4)
    refused("null pointer", proj_x=None)                      # no projection source and no q / k / v


@needs_lib
@pytest.mark.parametrize("heads", [4, 8])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_packed_permutation_round_trips(dtype, heads):
    hd, K = 72, 288
    N = 3 * heads * hd
    rows = qkv_attn_rows(heads, hd)
    assert len(rows) == heads * 256 and sorted(r for r in rows if r >= 0) == list(range(N))      # every row of W exactly once
    g = torch.Generator().manual_seed(7)
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
    # the q chunks' order: chunk row 8 g + 4 lh + e of chunk c holds q channel 32 c + 16 (g >> 1) + 8 lh + 4 (g & 1) + e, columns 72..79 zero rows
    for h in range(heads):
        for c in range(3):
            for s2 in range(2):
                for lh in range(2):
                    frag = [rows[h * 256 + 32 * c + 8 * (2 * s2 + (i >> 2)) + 4 * lh + (i & 3)] for i in range(8)]
                    d0 = 32 * c + 16 * s2 + 8 * lh
                    assert frag == [h * hd + d0 + i if d0 + i < hd else -1 for i in range(8)], (h, c, s2, lh)
