"""Which launches a Hiera trunk takes, decided apart from emitting them: the `CVMI_SAM_*` switches, the trunk's block structure, the packed weight
forms each block gets, and per block one `BlockRoute`.  Everything here is a pure function of shapes, dtype and switches -- no device, no buffers --
so the route of any configuration can be read (and is tested, tests/test_sam2_route_cpu.py) without a GPU.  `sam2.Sam2Weights._trunk` packs what
`block_packings` names; `sam2.Sam2Plan._block` emits what `route_block` returns."""
import os
from typing import NamedTuple, Optional

from ._lib import F32
from .engine import (hiera_mlp_supported, is16, qkv_attn16_supported, qkv_attn_supported, row_stats_supported, tok_linear_stats_parts,
                     tok_linear_supported)


# field -> (environment variable, who reads it, what "0" restores); every switch defaults to "1".  "weights": decides what Sam2Weights packs, read
# when the weights are built (a plan takes it from its weights); "plan": decides what Sam2Plan launches, read when the plan is built
SWITCH_TABLE = dict(
    fused_mlp=("CVMI_SAM_FUSED_MLP", "weights", "stages 1 - 2 MLP as fc1 + fc2 launches (no hiera_mlp / proj_mlp kernel)"),
    toklin=("CVMI_SAM_TOKLIN", "weights", "every short-K linear through the tiled GEMM behind a LayerNorm / cast launch (no tok_linear kernel)"),
    qlog2=("CVMI_SAM_QLOG2", "weights", "q rows without scale * log2(e) folded in; the attention kernels scale the scores themselves"),
    qkvattn=("CVMI_SAM_QKVATTN", "weights", "qkv and window attention as two launches in every block (also turns CVMI_SAM_QKVATTN16 off)"),
    qkvattn16=("CVMI_SAM_QKVATTN16", "weights", "qkv and window attention as two launches in the 4 x 4-window blocks of input width 288 alone"),
    qkvtok_trans=("CVMI_SAM_QKVTOK_TRANS", "plan", "the stage-transition blocks' qkv through the tiled GEMM behind a norm1 launch"),
    poolfuse=("CVMI_SAM_POOLFUSE", "plan", "a transition block's norm1, dimproj and 2 x 2 max-pool as three launches"),
    lnstats=("CVMI_SAM_LNSTATS", "plan", "every LayerNorm prologue computes its own statistics (no hand-over between launches)"),
    lnstats_fc2=("CVMI_SAM_LNSTATS_FC2", "plan", "stage-3 fc2 (tiled GEMM) hands no row statistics to the next block's norm1"),
    projmlp=("CVMI_SAM_PROJMLP", "plan", "attention proj and fused MLP as two launches"),
    neckcast=("CVMI_SAM_NECKCAST", "plan", "feat_s0 / feat_s1 through a cast launch and the tiled GEMM"),
    share_l0=("CVMI_SAM_SHARE_L0", "plan", "prompted decoder layer 0 on B * P repeated image streams (the repeat_embed launch)"),
)
SamSwitches = NamedTuple("SamSwitches", [(f, bool) for f in SWITCH_TABLE])      # one bool per row of the table, True = on
WEIGHT_SWITCHES = tuple(f for f, (_, reader, _) in SWITCH_TABLE.items() if reader == "weights")


def sam_switches():
    """The switches as the environment has them now."""
    return SamSwitches(**{f: os.environ.get(name, "1") != "0" for f, (name, _, _) in SWITCH_TABLE.items()})


class HieraBlock(NamedTuple):
    dim: int
    dim_out: int
    heads: int
    window: int        # 0: global attention
    q_pool: bool


def hiera_blocks(hiera):
    """(blocks, stage_ends) of a Hiera trunk: widths and heads double in the block after each stage's end, which (for the first three) also
    pools q 2 x 2; a stage's window holds through that block."""
    stages, ws = hiera["stages"], hiera["window_spec"]
    stage_ends = [sum(stages[:i]) - 1 for i in range(1, len(stages) + 1)]
    q_pool_blocks = [x + 1 for x in stage_ends[:-1]][:3]
    blocks, cur, dim, heads = [], 1, hiera["embed_dim"], hiera["num_heads"]
    for i in range(sum(stages)):
        dim_out, window = dim, 0 if i in hiera["global_att_blocks"] else ws[cur - 1]
        if i - 1 in stage_ends:
            dim_out, heads, cur = dim * 2, heads * 2, cur + 1
        if window > 0 and i in q_pool_blocks and window % 2:
            raise ValueError("q-pool block with odd window")
        blocks.append(HieraBlock(dim, dim_out, heads, window, i in q_pool_blocks))
        dim = dim_out
    return blocks, stage_ends


def block_packings(blocks, dtype, sw):
    """Keys of the packed forms the blocks get beside the tiled GEMM's: `b{i}.qkv` / `.proj` / `.fc1` / `.dimproj` (PackedTokLinear),
    `b{i}.qkv_attn` (PackedQkvAttn), `b{i}` and `b{i}.projmlp` (PackedHieraMlp, PackedProjMlp).  Packing knows no batch, so the kernels' row and
    window conditions are asked with counts every kernel accepts; `route_block` asks again with the plan's."""
    ROWS, NWIN = 256, 8            # stand-ins: one tok_linear workgroup's rows; a window count both qkv_attn (pairs) and qkv_attn16 (eights) take
    keys = set()
    tok = lambda K: sw.toklin and tok_linear_supported(K, dtype, ROWS)
    for i, b in enumerate(blocks):
        if tok(b.dim):
            keys.add(f"b{i}.qkv")
            if ((sw.qkvattn and qkv_attn_supported(b.dim, b.dim_out, b.heads, b.window, b.q_pool, dtype, NWIN))
                    or (sw.qkvattn and sw.qkvattn16 and qkv_attn16_supported(b.dim, b.dim_out, b.heads, b.window, b.q_pool, dtype, NWIN))):
                keys.add(f"b{i}.qkv_attn")
            if b.dim != b.dim_out:
                keys.add(f"b{i}.dimproj")
        if tok(b.dim_out):
            keys.add(f"b{i}.proj")
        if sw.fused_mlp and hiera_mlp_supported(b.dim_out, dtype):
            keys |= {f"b{i}", f"b{i}.projmlp"}
        elif tok(b.dim_out):
            keys.add(f"b{i}.fc1")
    return keys


class BlockRoute(NamedTuple):
    """Everything decided about one block's launches.  A statistics hand-over is None (not made) or its `parts`: 0 = [rows, 2] of (mean, rstd),
    P > 0 = [rows, P, 2] of per-slice (mean, sum of squared deviations)."""
    Hp: int
    Wp: int
    padded: bool
    OH: int
    OW: int
    nwin: int                     # attention batch: windows, or images of a global block
    nq: int
    nk: int
    q_log2: bool                  # cvmi_attn_desc.q_log2 of the block's attention launch: the q rows were packed with scale * log2(e) folded in
    norm1: Optional[str]          # "padded" | "plain" | None: fused into every launch that reads the normalised tokens
    dimproj: Optional[str]        # "tok_pool" (norm1 + dimproj + max-pool in one launch) | "gemm" (+ max-pool launch) | None: no width change
    qkv: str                      # "fused" into the attention launch | "tok" (tok_linear, norm1 fused) | "gemm"
    attn: str                     # "window" | "global" (whether the launch also projects qkv is `qkv`)
    proj: str                     # "fused" into the MLP launch | "tok" | "gemm"
    mlp: str                      # "fused" (hiera_mlp / proj_mlp) | "tok_fc1" (norm2 fused into fc1) | "gemm_fc1" (norm2 launch + GEMM); both + fc2 GEMM
    stats_in: Optional[int]       # statistics the previous block left for these rows' norm1
    stats_fc1: Optional[int]      # proj -> fc1 (norm2)
    stats_mlp: bool               # fused MLP -> the next block's norm1
    stats_fc2: Optional[int]      # fc2's row_stats -> the next block's norm1
    stats_next: Optional[tuple]   # (rows, parts) handed to the next block's route

    def launches(self, i):
        """[(label, kind)] in launch order.  A second statement of the order in which `Sam2Plan._block` emits, kept for the tests: the fixture
        test derives sequences from it without a GPU, and tests/test_sam2_route_gpu.py holds `_block` to it -- change the two together."""
        g = lambda *names: [(f"b{i}.{n}", "gemm") for n in names]
        out = [(f"b{i}.norm1", "layernorm")] if self.norm1 else []
        out += g("dimproj_pool") if self.dimproj == "tok_pool" else g("dimproj") + [(f"b{i}.pool", "pool")] if self.dimproj else []
        out += g("qkv") if self.qkv != "fused" else []
        out += [(f"b{i}.attn", "attn_global" if self.attn == "global" else "attn_window")]
        out += g("proj") if self.proj != "fused" else []
        if self.mlp == "fused":
            return out + [(f"b{i}.mlp", "mlp_fused")]
        return out + ([(f"b{i}.norm2", "layernorm")] if self.mlp == "gemm_fc1" else []) + g("fc1", "fc2")


def route_block(blocks, packed, i, B, H, W, dtype, av_fp8, sw, stats_prev):
    """Route of block i on a B x H x W token grid.  packed: `block_packings` of the weights; sw: the plan's switches; stats_prev: the previous
    block's `stats_next`."""
    b = blocks[i]
    dim, dout, ws = b.dim, b.dim_out, b.window
    # Hiera pads the NORMALISED tokens up to a window multiple (zeros), attends inside the padded windows and crops after the un-partition
    Hp, Wp = (H, W) if ws == 0 else (-(-H // ws) * ws, -(-W // ws) * ws)
    padded = (Hp, Wp) != (H, W)
    if b.q_pool and (ws == 0 or ws % 2 or Hp % 2 or Wp % 2):
        raise NotImplementedError("q-pool block needs an even window")
    rows = B * H * W
    tok_rows = not padded and rows % 256 == 0                  # token-stationary linears (tok_linear.hip) take 256-row workgroups
    tok_qkv = tok_rows and f"b{i}.qkv" in packed and (dim == dout or sw.qkvtok_trans)
    tok_pool = tok_rows and dim != dout and f"b{i}.dimproj" in packed and sw.poolfuse
    norm1 = "padded" if padded else "plain" if not tok_qkv or (dim != dout and not tok_pool) else None
    stats_in = stats_prev[1] if stats_prev is not None and stats_prev[0] == rows else None     # (written for exactly these rows)
    nwin = B * (Hp // ws) * (Wp // ws) if ws else B
    # qkv + window attention as ONE launch where a kernel is built for the block (stages 1 and 2); it reads (mean, rstd) statistics, not slices
    fuse_qkv = (tok_qkv and ws > 0 and f"b{i}.qkv_attn" in packed and not av_fp8 and not stats_in
                and (qkv_attn_supported(dim, dout, b.heads, ws, b.q_pool, dtype, nwin) or qkv_attn16_supported(dim, dout, b.heads, ws, b.q_pool, dtype, nwin)))
    OH, OW = (H // 2, W // 2) if b.q_pool else (H, W)
    orows = B * OH * OW
    tok_out = not padded and orows % 256 == 0
    fused_mlp = f"b{i}" in packed
    # norm2's statistics travel from the launch that writes x to the launch that normalises it (fc1 then reads x once, not twice)
    fwd = tok_out and f"b{i}.proj" in packed and not fused_mlp and f"b{i}.fc1" in packed and sw.lnstats
    # stages 1 / 2: proj as the prologue of the fused MLP launch; unpadded, the attention output is exactly the block's rows, dout wide
    fuse_proj = f"b{i}.projmlp" in packed and not padded and sw.projmlp
    nxt = blocks[i + 1] if i + 1 < len(blocks) else None
    nxt_qkv = nxt is not None and f"b{i + 1}.qkv" in packed
    stats_mlp = fused_mlp and nxt_qkv and sw.lnstats and orows % 256 == 0
    # a tiled GEMM hands the next block's norm1 raw per-slice sums (the 256 x 192 kernel: stage-3 fc2 shape); tok_linear adds them up
    stats_fc2 = (dout // 96 if not fused_mlp and nxt_qkv and nxt.dim == dout and tok_out and dtype != F32 and row_stats_supported(orows, dout, 4 * dout)
                 and sw.lnstats and sw.lnstats_fc2 else None)
    return BlockRoute(
        Hp=Hp, Wp=Wp, padded=padded, OH=OH, OW=OW, nwin=nwin, nq=H * W if not ws else (ws // 2) ** 2 if b.q_pool else ws * ws, nk=ws * ws if ws else H * W,
        q_log2=is16(dtype) and sw.qlog2, norm1=norm1, dimproj=None if dim == dout else "tok_pool" if tok_pool else "gemm",
        qkv="fused" if fuse_qkv else "tok" if tok_qkv else "gemm", attn="window" if ws else "global",
        proj="fused" if fuse_proj else "tok" if tok_out and f"b{i}.proj" in packed else "gemm",
        mlp="fused" if fused_mlp else "tok_fc1" if tok_out and f"b{i}.fc1" in packed else "gemm_fc1",
        stats_in=stats_in, stats_fc1=tok_linear_stats_parts(orows, dout, dout) if fwd else None, stats_mlp=stats_mlp, stats_fc2=stats_fc2,
        stats_next=(orows, 0) if stats_mlp else (orows, stats_fc2) if stats_fc2 is not None else None)


def route_trunk(hiera, image_size, B, dtype, av_fp8, sw, packed=None):
    """[BlockRoute] of a whole trunk, the statistics state threaded from block to block (packed: default what these switches pack)."""
    blocks, _ = hiera_blocks(hiera)
    packed = block_packings(blocks, dtype, sw) if packed is None else packed
    routes, H, W, stats = [], image_size // 4, image_size // 4, None
    for i in range(len(blocks)):
        r = route_block(blocks, packed, i, B, H, W, dtype, av_fp8, sw, stats)
        routes.append(r)
        H, W, stats = r.OH, r.OW, r.stats_next
    return routes
