"""The emitter against the route: Sam2Plan._block appends exactly the launches hiera_route.route_block names, and the library dispatches each to
the kernel the route's choice implies.  MINI144 at 256^2 (fused and unfused qkv and proj, the q-pool transitions, a global block, token-stationary
and tiled-GEMM linears) and SAM 2.1-tiny at 1024^2 (padded windows, nothing fused): the smallest shapes at which every arm of the route exists."""
import pytest
import torch

import sam2_route_cases as rc
from circuitvision_amd import hiera_route as hr

pytestmark = pytest.mark.gpu

CASES = [c for c in rc.CASES if c["id"] in ("mini144_f16_B2", "tiny_f16_B1")]


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_plan_emits_what_the_route_names(case):
    sp = rc.build_plan(case)
    wt = sp.wt
    routes = hr.route_trunk(wt.hiera, wt.image_size, sp.B, wt.dtype, bool(sp.av_fp8), sp.sw, wt.packed_keys)
    want = [lk for i, r in enumerate(routes) for lk in r.launches(i)]
    trunk = [(op[0], op[1]) for op in sp.plan.ops if rc.BLOCK_LABEL.fullmatch(op[0])]
    assert trunk == want
    first = [op[0] for op in sp.plan.ops].index(want[0][0])
    assert [(op[0], op[1]) for op in sp.plan.ops[first:first + len(want)]] == want            # one contiguous run, in order
    sp.x_in.t.normal_(generator=torch.Generator(device="cuda").manual_seed(0))
    torch.cuda.synchronize()
    timed = sp.plan.timed_eager(with_kernels=True)
    torch.cuda.synchronize()
    fused = ("qkv_attn64_kernel", "qkv_attn16_kernel", "proj_mlp_kernel")
    n_fused = 0
    for i, (r, launches) in enumerate(zip(routes, rc.trunk_blocks([(t[0], t[1], t[5]) for t in timed]))):
        for suffix, _, family in launches:
            assert rc.family_implied(suffix, family, r, wt.blocks[i].window), (i, suffix, family, r)
            n_fused += family + "_kernel" in fused
    kernels = {t[5].split("<")[0] for t in timed}
    if case["hiera"] == "MINI144":
        # blocks 0 - 1 on 8 x 8 windows, 2 - 3 on 4 x 4; proj rides in the MLP launch of 0 - 2; stage 3 on takes neither
        assert [r.qkv == "fused" for r in routes] == [True] * 4 + [False] * 4 and [r.proj == "fused" for r in routes] == [True] * 3 + [False] * 5
        assert set(fused) <= kernels and n_fused == 7
        assert {r.attn for r in routes} == {"window", "global"} and {r.qkv for r in routes} == {"fused", "tok", "gemm"} and {r.dimproj for r in routes} == {None, "tok_pool"}
    else:
        assert not set(fused) & kernels and n_fused == 0
        # windows of 14 on the 64-grid and 7 on the 32-grid do not divide; 8 on 256 and 4 on 128 do
        assert [r.padded for r in routes] == [b.window in (14, 7) for b in wt.blocks] and {r.dimproj for r in routes} == {None, "gemm"}
        assert {r.norm1 for r in routes} == {"padded", "plain"}
    assert torch.isfinite(sp.low_res).all()
