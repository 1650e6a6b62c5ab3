"""SAM 2.1 image path on the cvmi355 kernels: weight preparation (LoRA merge, constant folding),
launch plan, and the reference's boundary objects.

What it replaces:
  * `get_modified_sam2(...)` -> model with `.load_state_dict`, `.eval`, `.sam2_model.image_size`,
    `__call__(x[B,3,1024,1024]) -> (high_res[B,1,1024,1024], low_res[B,1,256,256], iou[B,1])`
    (/root/reference/src/sam2_infer.py:277-410, :220-275; caller circuit_analyzer.py:203-242, :349-351)
  * `SAM2Transforms(resolution, mask_threshold, max_hole_area, max_sprinkle_area)` with `__call__`
    and `postprocess_masks` (sam2_infer.py:29-128; caller circuit_analyzer.py:245-250, :347, :354)
  * `infer_masks(images)`: the batched entry point named by BASELINE.json's north_star.

Weight preparation (host, fp32, once): LoRA adapters merged (W' = W + (alpha/r) B A, rows B12); the
FPN lateral convs composed with conv_s0 / conv_s1 (no 256-channel 256^2 map is ever materialised);
FPN level 2 = lateral(stage 3) + nearest-2x lateral(stage 4) as ONE two-source GEMM with the learned
dense prompt added in its epilogue; every "+ positional encoding" of the two-way transformer folded
into constant post-projection residuals; Hiera's bicubic position embedding precomputed.

Numerics: the residual stream, LayerNorm statistics, softmax and all accumulators are fp32; in F16
mode GEMM / attention operands are fp16.  F32 mode runs everything on exact-f32 MFMA (parity mode).
"""
import ctypes
import hashlib
import math
import threading
from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as TF

from . import _lib
from ._lib import ACT_GELU, ACT_NONE, ACT_RELU, ACT_SIGMOID, BF16, F16, F32
from .engine import (ESIZE, TORCH_DTYPE, is16, Buf, PackedConv, PackedHieraMlp, PackedProjMlp, PackedQkvAttn, PackedTokLinear, Plan, Rows, make_attn_desc, op_attention,
                     op_call, op_cast, op_conv, op_hiera_mlp, op_layernorm, op_maxpool2, op_tok_linear, op_tok_linear_pool, require_gpu, tok_linear_supported)
from .decoder_route import route_decoder
from .hiera_route import WEIGHT_SWITCHES, block_packings, hiera_blocks, route_block, sam_switches

LOG2E = 1.4426950408889634
HIERA_L = dict(embed_dim=144, num_heads=2, stages=(2, 6, 36, 4), global_att_blocks=(23, 33, 43), window_spec=(8, 4, 16, 8))
HIERA_T = dict(embed_dim=96, num_heads=1, stages=(1, 2, 7, 2), global_att_blocks=(5, 7, 9), window_spec=(8, 4, 14, 7))

# circuit_analyzer.py:156-199 -- the 36 LoRA-wrapped modules of the fine-tuned checkpoint
LORA_TARGETS_REFERENCE = (
    [f"sam_mask_decoder.transformer.layers.{l}.{a}.{p}" for l in (0, 1) for a in ("self_attn", "cross_attn_token_to_image")
     for p in ("k_proj", "q_proj", "v_proj", "out_proj")]
    + [f"sam_mask_decoder.transformer.layers.{l}.mlp.layers.{j}" for l in (0, 1) for j in (0, 1)]
    + ["sam_mask_decoder.iou_prediction_head.layers.2", "sam_mask_decoder.conv_s0", "sam_mask_decoder.conv_s1",
       "image_encoder.neck.convs.2.conv", "image_encoder.neck.convs.3.conv",
       "image_encoder.trunk.blocks.44.attn.qkv", "image_encoder.trunk.blocks.44.mlp.layers.0", "image_encoder.trunk.blocks.44.proj",
       "image_encoder.trunk.blocks.47.attn.qkv", "image_encoder.trunk.blocks.47.mlp.layers.0"]
    + [f"sam_mask_decoder.transformer.layers.{l}.cross_attn_image_to_token.{p}" for l in (0, 1) for p in ("q_proj", "k_proj", "v_proj")])


# upstream PromptEncoder.mask_downscaling (mask_in_chans = 16): Conv2d(1,4,2,2) LayerNorm2d GELU Conv2d(4,16,2,2) LayerNorm2d GELU Conv2d(16,256,1)
MASK_DOWN = "sam_prompt_encoder.mask_downscaling"
MASK_DOWN_PARAMS = 4684                          # include/cvmi355.h CVMI_MASK_PROMPT_PARAMS


def mask_down_tensors():
    """(state-dict key, shape, synthetic kind) of the stack's ten tensors, in the order cvmi_mask_prompt_embed's parameter vector packs them."""
    return [(f"{MASK_DOWN}.0.weight", (4, 1, 2, 2), "w"), (f"{MASK_DOWN}.0.bias", (4,), "w"),
            (f"{MASK_DOWN}.1.weight", (4,), "gamma"), (f"{MASK_DOWN}.1.bias", (4,), "w"),
            (f"{MASK_DOWN}.3.weight", (16, 4, 2, 2), "w"), (f"{MASK_DOWN}.3.bias", (16,), "w"),
            (f"{MASK_DOWN}.4.weight", (16,), "gamma"), (f"{MASK_DOWN}.4.bias", (16,), "w"),
            (f"{MASK_DOWN}.6.weight", (256, 16, 1, 1), "w"), (f"{MASK_DOWN}.6.bias", (256,), "w")]


# ---- parameter sources ---------------------------------------------------------------------------------
class SamSyntheticParams:
    """Seeded synthetic weights in the fine-tuned checkpoint's own key format (PEFT names for LoRA
    targets, wrapper parameters at the top level).  `state_dict()` loads strictly into the oracle."""

    def __init__(self, seed=0, lora_targets=LORA_TARGETS_REFERENCE, r=4, alpha=16, std=0.02):
        self.seed, self.targets, self.r, self.scaling, self.std, self.sd = seed, set(lora_targets), r, alpha / r, std, {}
        self.mask_sd = {}              # sam_prompt_encoder.mask_downscaling.*: kept apart, `state_dict()` stays what the oracle loads strictly

    def _t(self, name, shape, kind="w"):
        sd = self.mask_sd if name.startswith(MASK_DOWN + ".") else self.sd
        if name in sd:
            assert tuple(sd[name].shape) == tuple(shape), (name, sd[name].shape, shape)
            return sd[name]
        h = int.from_bytes(hashlib.sha256(f"{self.seed}:{name}".encode()).digest()[:8], "little") & 0x7FFFFFFFFFFFFFFF
        g = torch.Generator().manual_seed(h)
        if kind == "gamma":
            t = torch.empty(shape).uniform_(0.8, 1.2, generator=g)
        elif kind == "unit":
            t = torch.empty(shape).normal_(0, 1.0, generator=g)
        elif kind == "refine":
            t = torch.empty(shape).normal_(0, 0.2, generator=g)
        else:
            t = torch.empty(shape).normal_(0, self.std, generator=g).clamp_(-2 * self.std, 2 * self.std)
        sd[name] = t
        return t

    def weight(self, mod, shape):
        """Merged weight of module `mod` (Linear [out,in] or Conv [out,in,kh,kw])."""
        if mod in self.targets:
            w = self._t(f"{mod}.base_layer.weight", shape)
            a_shape = (self.r, shape[1]) + tuple(shape[2:])
            b_shape = (shape[0], self.r) + (1,) * (len(shape) - 2)
            A = self._t(f"{mod}.lora_A.default.weight", a_shape)
            Bm = self._t(f"{mod}.lora_B.default.weight", b_shape)
            delta = (Bm.reshape(shape[0], self.r) @ A.reshape(self.r, -1)).reshape(shape)
            return w + self.scaling * delta
        return self._t(f"{mod}.weight", shape)

    def bias(self, mod, n):
        return self._t(f"{mod}.base_layer.bias" if mod in self.targets else f"{mod}.bias", (n,))

    def tensor(self, name, shape, kind="w"):
        return self._t(name, shape, kind)

    def state_dict(self):
        return dict(self.sd)

    def mask_prompt_state_dict(self):
        """The ten tensors of `sam_prompt_encoder.mask_downscaling` (mask prompts, `infer_masks(mask_input=...)`) under their upstream
        names.  Not part of `state_dict()`: the oracle restates the prompt encoder without that stack."""
        for name, shape, kind in mask_down_tensors():
            self._t(name, shape, kind)
        return dict(self.mask_sd)


class SamBlankParams:
    """A rank that holds NO checkpoint: every tensor reads as zeros, so `Sam2Weights` allocates the packed buffers at their final shapes
    (no random generation, no file) and `distributed.broadcast_weights` fills them from the rank that read the checkpoint."""

    def weight(self, mod, shape):
        return torch.zeros(shape)

    def bias(self, mod, n):
        return torch.zeros(n)

    def tensor(self, name, shape, kind="w"):
        return torch.zeros(shape)

    def state_dict(self):
        return {}


class SamStateDictParams:
    """A real checkpoint: flat state_dict (optionally under 'state_dict'), PEFT key names with the
    `sam2_model.base_model.model.` prefix (sam2_infer.py:396), wrapper parameters at the top level."""

    PREFIXES = ("sam2_model.base_model.model.", "sam2_model.")

    def __init__(self, sd, r=4, alpha=16):
        self.scaling = alpha / r
        self.sd = {}
        for k, v in sd.items():
            for p in self.PREFIXES:
                if k.startswith(p):
                    k = k[len(p):]
                    break
            self.sd[k] = v.detach().float().cpu()

    def _get(self, name, shape):
        t = self.sd[name]
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name}: checkpoint shape {tuple(t.shape)} != expected {tuple(shape)}")
        return t

    def weight(self, mod, shape):
        if f"{mod}.base_layer.weight" in self.sd:
            w = self._get(f"{mod}.base_layer.weight", shape)
            A, Bm = self.sd[f"{mod}.lora_A.default.weight"], self.sd[f"{mod}.lora_B.default.weight"]
            r = A.shape[0]
            return w + self.scaling * (Bm.reshape(shape[0], r) @ A.reshape(r, -1)).reshape(shape)
        return self._get(f"{mod}.weight", shape)

    def bias(self, mod, n):
        k = f"{mod}.base_layer.bias" if f"{mod}.base_layer.bias" in self.sd else f"{mod}.bias"
        return self._get(k, (n,))

    def tensor(self, name, shape, kind="w"):
        return self._get(name, shape)


class SamBaseCheckpointParams(SamStateDictParams):
    """The SAM 2 base checkpoint (`{'model': state_dict}`, plain upstream keys) that `build_sam2` loads
    (sam2_infer.py:333).  It has no LoRA tensors and none of the wrapper's own parameters; those start, as in the
    reference before the fine-tuned state dict is loaded, from `torch.randn` (sam2_infer.py:207-209) / default conv
    init -- seeded here so that runs are reproducible."""

    WRAPPER = ("dense_embedding", "sparse_embedding", "refinement_layer.")

    def __init__(self, sd, seed=0):
        super().__init__(sd.get("model", sd) if isinstance(sd, dict) else sd)
        self.seed = seed

    def tensor(self, name, shape, kind="w"):
        if name in self.sd:
            return self._get(name, shape)
        if name.startswith(self.WRAPPER):
            h = int.from_bytes(hashlib.sha256(f"{self.seed}:{name}".encode()).digest()[:8], "little") & 0x7FFFFFFFFFFFFFFF
            g = torch.Generator().manual_seed(h)
            t = torch.empty(shape).normal_(0, 1.0 if "embedding" in name else 0.1, generator=g)
            self.sd[name] = t
            return t
        raise KeyError(name)


# ---- prepared weights -----------------------------------------------------------------------------------------
def _lin(w):
    return w.reshape(w.shape[0], w.shape[1], 1, 1)


class Sam2Weights:
    def __init__(self, params, hiera=HIERA_L, image_size=1024, dtype=F16, device="cuda", use_refinement=True,
                 refinement_kernels=(3, 5, 7, 11), embedding_r=4):
        self.p, self.hiera, self.image_size, self.dtype, self.device = params, hiera, image_size, dtype, device
        self.use_refinement, self.kernels = use_refinement, tuple(refinement_kernels)
        self.pc, self.ln, self.const, self.mlp, self.tl = {}, {}, {}, {}, {}
        self.sw = sw = sam_switches()                      # (A/B switches, hiera_route.SWITCH_TABLE; the weight-level ones decide what is packed)
        self.fused_mlp, self.use_tok, self.qkv_attn, self.qkv_attn16 = sw.fused_mlp, sw.toklin, sw.qkvattn, sw.qkvattn and sw.qkvattn16
        # Hiera q rows carry scale * log2(e) (16-bit plans): see _linear(row_scale=) and cvmi_attn_desc.q_log2
        self.q_log2 = is16(dtype) and sw.qlog2
        self.param_bytes = 0
        self.flops_per_image = 0
        self._trunk()
        self._neck_and_prompts(embedding_r)
        self._decoder()
        self._refinement()

    # -- helpers
    def _pack(self, key, w4, b):
        pc = PackedConv(w4, b, self.dtype, self.device)
        self.pc[key] = pc
        self.param_bytes += pc.param_bytes
        return pc

    def _linear(self, key, mod, cout, cin, row_scale=None, heads=0):
        w, b = self.p.weight(mod, (cout, cin)), self.p.bias(mod, cout)
        if row_scale is not None:
            # (rows, factor): the attention scale * log2(e) folded into the q rows of a qkv projection, in fp32 before the weights are rounded
            # to the operand type -- the attention kernels then take exp2 of q k^T as it stands (cvmi_attn_desc.q_log2)
            n, f = row_scale
            w, b = w.clone(), b.clone()
            w[:n] *= f
            b[:n] *= f
        if key in self.packed_keys:
            # short-K Hiera linears also in the token-stationary kernel's fragment order (tok_linear.hip); the plan picks it
            # whenever its row count is a multiple of 256
            self.tl[key] = PackedTokLinear(w, b, self.device, self.dtype)
        if key + "_attn" in self.packed_keys:
            # ... and, rows permuted head by head, for the fused qkv + window-attention launch (engine.PackedQkvAttn)
            self.tl[key + "_attn"] = PackedQkvAttn(w, b, heads, self.device, self.dtype)
        return self._pack(key, _lin(w), b)

    def _norm(self, key, mod, c):
        self.ln[key] = (self.p.tensor(f"{mod}.weight", (c,), "gamma").float().to(self.device),
                        self.p.tensor(f"{mod}.bias", (c,)).float().to(self.device))

    def _trunk(self):
        h = self.hiera
        E, stages, ws = h["embed_dim"], h["stages"], h["window_spec"]
        T = "image_encoder.trunk"
        # PatchEmbed 7x7 / s4 / pad 3 on the space-to-depth(4) image: window row ky = 0..2 sits in block row -1 (sub-row
        # ky + 1), ky = 3..6 in block row 0 (sub-row ky - 3); same for columns -> a 2x2 conv over 48 channels
        w7 = self.p.weight(f"{T}.patch_embed.proj", (E, 3, 7, 7))
        w2 = torch.zeros(E, 48, 2, 2)
        m = {k: ((0, k + 1) if k < 3 else (1, k - 3)) for k in range(7)}
        for ky in range(7):
            for kx in range(7):
                (ty, sy), (tx, sx) = m[ky], m[kx]
                w2[:, (sy * 4 + sx) * 3:(sy * 4 + sx) * 3 + 3, ty, tx] = w7[:, :, ky, kx]
        self._pack("patch_embed", w2, self.p.bias(f"{T}.patch_embed.proj", E))
        g = self.image_size // 4
        pos = TF.interpolate(self.p.tensor(f"{T}.pos_embed", (1, E, 7, 7)), size=(g, g), mode="bicubic")
        win = self.p.tensor(f"{T}.pos_embed_window", (1, E, ws[0], ws[0]))
        pos = pos + win.tile([1, 1, g // ws[0], g // ws[0]])
        self.const["pos_embed"] = pos.permute(0, 2, 3, 1).reshape(g * g, E).contiguous().float().to(self.device)   # f32 residual stream
        self.blocks, self.stage_ends = hiera_blocks(h)
        self.packed_keys = block_packings(self.blocks, self.dtype, self.sw)      # keys of the packed forms beside the tiled GEMM's; Sam2Plan routes by them
        for i, (dim, dim_out, heads, _, _) in enumerate(self.blocks):
            b = f"{T}.blocks.{i}"
            self._norm(f"b{i}.norm1", f"{b}.norm1", dim)
            self._linear(f"b{i}.qkv", f"{b}.attn.qkv", 3 * dim_out, dim, heads=heads,
                         row_scale=(dim_out, (dim_out // heads) ** -0.5 * LOG2E) if self.q_log2 else None)
            self._linear(f"b{i}.proj", f"{b}.attn.proj", dim_out, dim_out)
            self._norm(f"b{i}.norm2", f"{b}.norm2", dim_out)
            if f"b{i}" in self.packed_keys:
                # stages 1 / 2: norm2 + fc1 + GELU + fc2 + residual as ONE launch (hiera_mlp.hip); weights in fragment order
                self.mlp[f"b{i}"] = PackedHieraMlp(self.p.weight(f"{b}.mlp.layers.0", (4 * dim_out, dim_out)), self.p.bias(f"{b}.mlp.layers.0", 4 * dim_out),
                                                   self.p.weight(f"{b}.mlp.layers.1", (dim_out, 4 * dim_out)), self.p.bias(f"{b}.mlp.layers.1", dim_out),
                                                   self.device, self.dtype)
                self.param_bytes += self.mlp[f"b{i}"].param_bytes
                # ... and, behind the attention projection, for the launch that runs proj + MLP together (proj_mlp.hpp); the same parameters
                # a second time, so param_bytes stays
                self.mlp[f"b{i}.projmlp"] = PackedProjMlp(self.p.weight(f"{b}.attn.proj", (dim_out, dim_out)), self.p.bias(f"{b}.attn.proj", dim_out),
                                                          self.p.weight(f"{b}.mlp.layers.0", (4 * dim_out, dim_out)), self.p.bias(f"{b}.mlp.layers.0", 4 * dim_out),
                                                          self.p.weight(f"{b}.mlp.layers.1", (dim_out, 4 * dim_out)), self.p.bias(f"{b}.mlp.layers.1", dim_out),
                                                          self.device, self.dtype)
            else:
                self._linear(f"b{i}.fc1", f"{b}.mlp.layers.0", 4 * dim_out, dim_out)
                self._linear(f"b{i}.fc2", f"{b}.mlp.layers.1", dim_out, 4 * dim_out)
            if dim != dim_out:
                self._linear(f"b{i}.dimproj", f"{b}.proj", dim_out, dim)
        self.stage_dims = [E * 2 ** s for s in range(len(stages))]

    def _neck_and_prompts(self, embedding_r):
        N, D = "image_encoder.neck", "sam_mask_decoder"
        c = self.stage_dims                                   # [144, 288, 576, 1152]
        wn = [self.p.weight(f"{N}.convs.{j}.conv", (256, c[3 - j], 1, 1)).reshape(256, -1) for j in range(4)]
        bn = [self.p.bias(f"{N}.convs.{j}.conv", 256) for j in range(4)]
        ws0, bs0 = self.p.weight(f"{D}.conv_s0", (32, 256, 1, 1)).reshape(32, 256), self.p.bias(f"{D}.conv_s0", 32)
        ws1, bs1 = self.p.weight(f"{D}.conv_s1", (64, 256, 1, 1)).reshape(64, 256), self.p.bias(f"{D}.conv_s1", 64)
        # level 0 (256^2, 144 ch): conv_s0 o lateral ; level 1 (128^2, 288 ch): conv_s1 o lateral
        self._pack("feat_s0", _lin(ws0 @ wn[3]), ws0 @ bn[3] + bs0)
        self._pack("feat_s1", _lin(ws1 @ wn[2]), ws1 @ bn[2] + bs1)
        if self.use_tok and is16(self.dtype):                    # ... and for tok_linear's plain-f32-input form: the stage outputs need no cast pass
            for key, w_, b_ in (("feat_s0", ws0 @ wn[3], ws0 @ bn[3] + bs0), ("feat_s1", ws1 @ wn[2], ws1 @ bn[2] + bs1)):
                if tok_linear_supported(w_.shape[1], self.dtype, 256) and w_.shape[1] <= 288:
                    self.tl[key] = PackedTokLinear(w_, b_, self.device, self.dtype)
        # level 2 (64^2): lateral(stage 3, 576) + nearest2x(lateral(stage 4, 1152)) as one K-concatenated GEMM
        self._pack("embed", _lin(torch.cat((wn[1], wn[0]), 1)), bn[1] + bn[0])
        fs = self.image_size // 16
        e1 = self.p.tensor("dense_embedding1", (1, 256, embedding_r), "unit")
        e2 = self.p.tensor("dense_embedding2", (1, embedding_r, fs * fs), "unit")
        dense = (e1 @ e2).view(256, fs * fs).t().contiguous()                       # [pixels, 256]  (sam2_infer.py:250)
        self.const["dense"] = dense.float().to(self.device)
        G = self.p.tensor("sam_prompt_encoder.pe_layer.positional_encoding_gaussian_matrix", (2, 128), "unit")
        yy, xx = torch.meshgrid((torch.arange(fs, dtype=torch.float32) + 0.5) / fs, (torch.arange(fs, dtype=torch.float32) + 0.5) / fs, indexing="ij")
        cpe = 2 * math.pi * ((2 * torch.stack((xx, yy), -1) - 1) @ G)
        self.key_pe = torch.cat((torch.sin(cpe), torch.cos(cpe)), -1).reshape(fs * fs, 256)      # get_dense_pe(), [pixels, 256]
        self.sparse = self.p.tensor("sparse_embedding", (1, 32, 256), "unit")[0]
        # upstream prompt encoder (box / point prompts, `infer_masks(images, boxes)`): label table, no-mask dense
        # embedding and the predictor's no_mem_embed, the last two folded into the embed GEMM's bias
        PE = "sam_prompt_encoder"
        try:
            table = torch.cat([self.p.tensor(f"{PE}.not_a_point_embed.weight", (1, 256), "unit")]
                              + [self.p.tensor(f"{PE}.point_embeddings.{i}.weight", (1, 256), "unit") for i in range(4)], 0)
            no_mask = self.p.tensor(f"{PE}.no_mask_embed.weight", (1, 256), "unit")[0]
            no_mem = self.p.tensor("no_mem_embed", (1, 1, 256), "unit").reshape(256)
        except KeyError:
            self.prompt_ok = self.mask_prompt_ok = False      # a checkpoint stripped of the prompt encoder: learned-prompt path only
            return
        self.prompt_ok = True
        self._pack("embed_box", _lin(torch.cat((wn[1], wn[0]), 1)), bn[1] + bn[0] + no_mask + no_mem)
        self.const["prompt_table"] = table.float().contiguous().to(self.device)
        self.const["gauss"] = G.float().contiguous().to(self.device)
        # mask prompts (`infer_masks(mask_input=...)`): mask_downscaling packed for cvmi_mask_prompt_embed.  The last bias carries
        # - no_mask_embed: the embed GEMM above keeps its bias, and a masked pair's dense prompt REPLACES no_mask_embed
        try:
            parts = [self.p.tensor(name, shape, kind).float().reshape(-1) for name, shape, kind in mask_down_tensors()]
        except KeyError:
            self.mask_prompt_ok = False             # a checkpoint stripped of mask_downscaling: boxes and clicks only
            return
        self.mask_prompt_ok = True
        parts[-1] = parts[-1] - no_mask.float()
        self.const["mask_down"] = torch.cat(parts).contiguous().to(self.device)
        assert self.const["mask_down"].numel() == MASK_DOWN_PARAMS

    def _attn(self, key, mod, inner, q_pe=None, k_pe=None):
        """One Attention module.  q / k / v projections packed separately; constants (x + pe) W^T folded."""
        d = {}
        for nm in ("q_proj", "k_proj", "v_proj"):
            d[nm] = (self.p.weight(f"{mod}.{nm}", (inner, 256)), self.p.bias(f"{mod}.{nm}", inner))
        self._linear(f"{key}.out", f"{mod}.out_proj", 256, inner)
        return d

    def _decoder(self):
        D = "sam_mask_decoder"
        dev, od = self.device, TORCH_DTYPE[self.dtype]
        tokens = torch.cat((self.p.tensor(f"{D}.obj_score_token.weight", (1, 256), "unit"), self.p.tensor(f"{D}.iou_token.weight", (1, 256), "unit"),
                            self.p.tensor(f"{D}.mask_tokens.weight", (4, 256), "unit"), self.sparse), 0)          # [38, 256]
        self.tokens = tokens
        self.const["tokens"] = tokens.float().to(dev)
        kpe = self.key_pe
        self.n_tok = tokens.shape[0]
        self._sa_w, self._x_w = {}, {}

        def cres(t):                       # constant residual in the GEMM's output dtype
            return t.contiguous().to(od).to(dev)

        for l in (0, 1):
            L = f"{D}.transformer.layers.{l}"
            # self attention: q, k (+ token pe unless layer 0), v from the same queries -> one GEMM of N = 768
            sa = self._attn(f"l{l}.sa", f"{L}.self_attn", 256)
            self._sa_w[l] = (sa["q_proj"][0], sa["k_proj"][0])
            w = torch.cat([sa[n][0] for n in ("q_proj", "k_proj", "v_proj")], 0)
            b = torch.cat([sa[n][1] for n in ("q_proj", "k_proj", "v_proj")], 0)
            self._pack(f"l{l}.sa.qkv", _lin(w), b)
            if l > 0:
                pe = torch.cat((tokens @ sa["q_proj"][0].t(), tokens @ sa["k_proj"][0].t(), torch.zeros(self.n_tok, 256)), 1)
                self.const[f"l{l}.sa.qkv_pe"] = cres(pe)
            self._norm(f"l{l}.norm1", f"{L}.norm1", 256)
            # token -> image cross attention (internal dim 128)
            t2i = self._attn(f"l{l}.t2i", f"{L}.cross_attn_token_to_image", 128)
            self._pack(f"l{l}.t2i.q", _lin(t2i["q_proj"][0]), t2i["q_proj"][1])
            self.const[f"l{l}.t2i.q_pe"] = cres(tokens @ t2i["q_proj"][0].t())
            self._pack(f"l{l}.t2i.kv", _lin(torch.cat((t2i["k_proj"][0], t2i["v_proj"][0]), 0)), torch.cat((t2i["k_proj"][1], t2i["v_proj"][1]), 0))
            self.const[f"l{l}.t2i.kv_pe"] = cres(torch.cat((kpe @ t2i["k_proj"][0].t(), torch.zeros(kpe.shape[0], 128)), 1))
            self._norm(f"l{l}.norm2", f"{L}.norm2", 256)
            self._linear(f"l{l}.mlp1", f"{L}.mlp.layers.0", 2048, 256)
            self._linear(f"l{l}.mlp2", f"{L}.mlp.layers.1", 256, 2048)
            self._norm(f"l{l}.norm3", f"{L}.norm3", 256)
            # image -> token cross attention: q from keys (+ key pe), k from queries (+ token pe), v from queries
            i2t = self._attn(f"l{l}.i2t", f"{L}.cross_attn_image_to_token", 128)
            self._pack(f"l{l}.i2t.q", _lin(i2t["q_proj"][0]), i2t["q_proj"][1])
            self.const[f"l{l}.i2t.q_pe"] = cres(kpe @ i2t["q_proj"][0].t())
            self._pack(f"l{l}.i2t.kv", _lin(torch.cat((i2t["k_proj"][0], i2t["v_proj"][0]), 0)), torch.cat((i2t["k_proj"][1], i2t["v_proj"][1]), 0))
            self.const[f"l{l}.i2t.kv_pe"] = cres(torch.cat((tokens @ i2t["k_proj"][0].t(), torch.zeros(self.n_tok, 128)), 1))
            self._norm(f"l{l}.norm4", f"{L}.norm4", 256)
            self._x_w[l] = {"t2i.q": t2i["q_proj"][0], "i2t.k": i2t["k_proj"][0]}
        F_ = f"{D}.transformer.final_attn_token_to_image"
        fa = self._attn("final", F_, 128)
        # prompted mode: the token PE is per prompt, so (tokens0 @ W^T) is one run-time GEMM whose column groups are
        # the residuals the constant-folded path reads from `const[...]`
        zeros = lambda n: torch.zeros(n, 256)
        groups = [("l1.sa.qkv_pe", torch.cat((self._sa_w[1][0], self._sa_w[1][1], zeros(256)), 0))]
        for l in (0, 1):
            groups.append((f"l{l}.t2i.q_pe", self._x_w[l]["t2i.q"]))
            groups.append((f"l{l}.i2t.kv_pe", torch.cat((self._x_w[l]["i2t.k"], zeros(128)), 0)))
        groups.append(("final.q_pe", fa["q_proj"][0]))
        self.pe_off, off = {}, 0
        for name, w in groups:
            self.pe_off[name] = (off, w.shape[0])
            off += w.shape[0]
        self._pack("token_pe", _lin(torch.cat([w for _, w in groups], 0)), torch.zeros(off))
        self.const["out_tokens"] = tokens[:6].float().contiguous().to(dev)
        self._pack("final.q", _lin(fa["q_proj"][0]), fa["q_proj"][1])
        self.const["final.q_pe"] = cres(tokens @ fa["q_proj"][0].t())
        self._pack("final.kv", _lin(torch.cat((fa["k_proj"][0], fa["v_proj"][0]), 0)), torch.cat((fa["k_proj"][1], fa["v_proj"][1]), 0))
        self.const["final.kv_pe"] = cres(torch.cat((kpe @ fa["k_proj"][0].t(), torch.zeros(kpe.shape[0], 128)), 1))
        self._norm("norm_final", f"{D}.transformer.norm_final_attn", 256)
        # upscaling: ConvTranspose2d(k=2, s=2) weights [Cin, Cout, 2, 2] -> GEMM rows n = (dy*2+dx)*Cout + co
        for key, mod, cin, cout in (("up1", f"{D}.output_upscaling.0", 256, 64), ("up2", f"{D}.output_upscaling.3", 64, 32)):
            w = self.p.weight(mod, (cin, cout, 2, 2))
            b = self.p.bias(mod, cout)
            self._pack(key, _lin(w.permute(2, 3, 1, 0).reshape(4 * cout, cin)), b.repeat(4))
        self._norm("up_ln", f"{D}.output_upscaling.1", 64)
        for i in range(4):
            for j, (co, ci) in enumerate(((256, 256), (256, 256), (32, 256))):
                self._linear(f"hyper{i}.{j}", f"{D}.output_hypernetworks_mlps.{i}.layers.{j}", co, ci)
        for j, (co, ci) in enumerate(((256, 256), (256, 256), (4, 256))):
            self._linear(f"iou.{j}", f"{D}.iou_prediction_head.layers.{j}", co, ci)
        for j, (co, ci) in enumerate(((256, 256), (256, 256), (1, 256))):     # pred_obj_score_head: loaded (strictness), unused by the wrapper
            self.p.weight(f"{D}.pred_obj_score_head.layers.{j}", (co, ci)); self.p.bias(f"{D}.pred_obj_score_head.layers.{j}", co)
        # host-side intermediates of the constant folding above: no forward pass reads them, and a rank that receives its weights by
        # broadcast never has them (tests/test_distributed_cpu.py checks that everything left on this object is in the broadcast)
        del self.key_pe, self.sparse, self._sa_w, self._x_w, self.tokens

    def _refinement(self):
        if not self.use_refinement:
            self.refine_params = None
            return
        parts = []
        for j, k in enumerate(self.kernels):
            parts.append(self.p.tensor(f"refinement_layer.conv_branches.{j}.weight", (4, 1, k, k), "refine").reshape(-1))
            parts.append(self.p.tensor(f"refinement_layer.conv_branches.{j}.bias", (4,), "refine"))
        parts.append(self.p.tensor("refinement_layer.combiner_conv.weight", (1, 4 * len(self.kernels), 1, 1), "refine").reshape(-1))
        parts.append(self.p.tensor("refinement_layer.combiner_conv.bias", (1,), "refine"))
        self.refine_params = torch.cat([t.float() for t in parts]).to(self.device)


# The image of decoder batch entry n, for a launch that reads a per-image tensor: n // rep (a prompts = P plan: rep = P), else table[n] (a pairs plan's
# `pair_image`), else n itself (0 and None).  The fields are the kernels' `*_bdiv` / `res_rep` and `*_bmap` / `res_map` arguments.
_PairMap = namedtuple("_PairMap", "rep table")
_PER_PAIR = _PairMap(0, None)


class Sam2Plan:
    """Launch plan for B images: x [B, R, R, 3] (NHWC, normalised) -> high_res, low_res, iou.

    prompts = 0: the reference's learned-prompt wrapper forward (one mask per image, sam2_infer.py:220-275).
    prompts = P > 0: upstream prompting, P prompts of `points` labelled points per image (a box = 2 corners + 1
    padding point); the caller fills `coords` [B*P, points, 2] / `labels` [B*P, points] before each run and the decoder
    runs on B*P (image, prompt) pairs, image-major (MaskDecoder repeat_image=True); outputs are [B*P, 1, ...].
    mask_prompt (prompts > 0): every pair also carries a mask prompt, low-res logits the caller writes to `mask_in` [B*P, R/4, R/4]
    before each run (upstream `mask_input`); the image stream then differs per pair from the start, so layer 0 runs unshared.
    multimask (prompts > 0): upstream multimask_output=True -- mask tokens 1..3 and their IoU heads in token order, no stability
    fallback; outputs are [B*P, 3, ...].
    pairs = cap > 0 (in the place of prompts): the decoder runs on `cap` (image, prompt) pairs whose images the caller names in `pair_image`
    (device int32 [cap], written beside `coords` / `labels` / `mask_in` before each run; every value must lie in [0, B) -- the kernels read
    the table as it is): any number of prompts per image, in any order.  Everything that finds a pair's image as b / P in a prompts = P plan
    reads the table instead (the gather in the place of the repeat pass, layer 0's shared tensors, the up1 / up2 residuals); the table is
    data, so one captured plan serves every distribution of `cap` pairs over the B images.
    stage: "full" (default) is all of the above in one plan.  The other two cut it at the seam between `embed` and the first decoder launch -- the
    predictor's set_image / predict split:
      "encode"  stem, Hiera blocks, neck and BOTH forms of the embed GEMM (no prompt arguments): `feat_s0`, `feat_s1`, `emb` (the prompted form; None
                for a checkpoint without a prompt encoder) and `keys0` (the learned-prompt form) are its outputs
      "decode"  no `x_in`, no trunk, no neck: `feat_s0`, `feat_s1` and `emb` (prompted routes) or `keys0` (the `dense` stream) are INPUT buffers of
                the shapes and types the full plan has there, written by the caller before each run; the launches are the route's
                `decoder_launches()`, emitted by the same functions.  The decoder updates `keys0` in place: it is re-staged before EVERY run,
                the one `capture()` makes included."""

    def __init__(self, wt, B, stream, dynamic_multimask_via_stability=True, prompts=0, points=3, high_res=True, attn="16", mask_prompt=False,
                 multimask=False, pairs=0, stage="full"):
        """attn = "fp8" (16-bit plans only; BASELINE configs[4]): the AV contraction of Hiera's 256-key windows and global blocks runs on the
        block-scaled fp8 MFMA (cvmi_attn_desc.av_fp8); "16": operands in the plan's 16-bit type (default)."""
        self.wt, self.B, self.dt, self.dev = wt, B, wt.dtype, wt.device
        if attn not in ("16", "fp8") or (attn == "fp8" and not is16(wt.dtype)):
            raise ValueError("attn must be '16' or 'fp8' (fp8 needs an fp16 / bf16 plan)")
        self.av_fp8 = 1 if attn == "fp8" else 0
        if stage not in ("full", "encode", "decode"):
            raise ValueError("stage must be 'full', 'encode' or 'decode'")
        if stage == "encode" and (prompts or pairs or mask_prompt or multimask):
            raise ValueError("an encode plan takes no prompt arguments (it writes both forms of the embedding)")
        self.stage = stage
        self.sw = sam_switches()._replace(**{f: getattr(wt.sw, f) for f in WEIGHT_SWITCHES})      # plan-level switches as set now, weight-level as packed
        self.P, self.K = prompts, points
        # everything after the trunk is routed here (the route checks the prompt arguments), before anything is allocated; _neck_decoder emits it
        self.droute = route_decoder(wt.dtype, B, wt.image_size, self.sw, prompts=prompts, pairs=pairs, points=points, mask_prompt=mask_prompt,
                                    multimask=multimask, high_res=high_res, refine=wt.refine_params is not None,
                                    neck_tok=("feat_s0" in wt.tl, "feat_s1" in wt.tl), stage_dims=wt.stage_dims, n_tok=wt.n_tok)
        self.pairs = int(pairs)
        if self.droute.prompted and not wt.prompt_ok:
            raise _lib.CvmiError("this checkpoint carries no sam_prompt_encoder tensors: box / point prompts are unavailable")
        if mask_prompt and not wt.mask_prompt_ok:
            raise _lib.CvmiError("this checkpoint carries no sam_prompt_encoder.mask_downscaling tensors: mask prompts are unavailable")
        self.mask_prompt, self.multimask, self.share_l0 = bool(mask_prompt), bool(multimask), self.droute.stream == "shared"
        self.plan = Plan(stream)
        self.pool = {}
        self.dynamic = dynamic_multimask_via_stability
        self.act_bytes = 0
        self._build()
        torch.cuda.synchronize()

    def buf(self, H, W, C, dtype=None, tag=None, zero=False, batch=None):
        """Scratch buffers are shared between blocks of equal shape (launches are stream-ordered)."""
        dtype = self.dt if dtype is None else dtype
        batch = self.B if batch is None else batch
        key = (batch, H, W, C, dtype, tag)
        if tag is None or key not in self.pool:
            b = Buf(batch, H, W, C, dtype, self.dev, zero=zero)
            self.act_bytes += b.nbytes
            if tag is None:
                return b
            self.pool[key] = b
        return self.pool[key]

    def gemm(self, label, key, src, dst, act=ACT_NONE, res=None, kind="gemm", **kw):
        srcs = src if isinstance(src, list) else [(src, 0)]
        op_conv(self.plan, label, self.wt.pc[key], srcs, dst, act=act, res=res, kind=kind, **kw)

    def _build(self):
        wt, B = self.wt, self.B
        R = wt.image_size
        if self.stage == "decode":
            return self._decode_inputs(self.droute)
        g = R // 4
        self.x_in = Buf(B, R, R, 3, self.dt, self.dev, zero=True)
        E = wt.hiera["embed_dim"]
        x = self.buf(g, g, E, F32)
        pos = wt.const["pos_embed"]
        self.plan.keep.append(pos)
        xs = Buf(B, g, g, 48, self.dt, self.dev)
        lib = _lib.load()
        op_call(self.plan, "s2d4", "stem", lib.cvmi_space_to_depth4, (self.x_in.t.data_ptr(), xs.t.data_ptr(), B, R, R, self.dt),
                keep=(self.x_in, xs), bytes_=2 * self.x_in.nbytes)
        op_conv(self.plan, "patch_embed", wt.pc["patch_embed"], [(xs.view(), 0)], x.view(), stride=1, pad=1, out_hw=(g, g),
                res=_ConstView(pos, E), res_mod=g * g, kind="stem")
        H = W = g
        stage_out = []
        state, stats = None, None                 # LayerNorm statistics a block leaves for the next block's norm1: the route's (rows, parts) and the tensor
        for i in range(len(wt.blocks)):
            route = route_block(wt.blocks, wt.packed_keys, i, B, H, W, self.dt, self.av_fp8, self.sw, state)
            x, stats = self._block(i, route, x, H, W, stats)
            H, W, state = route.OH, route.OW, route.stats_next
            if i in wt.stage_ends:
                stage_out.append(x)
        self.stage_out = stage_out
        self._neck_decoder(stage_out)

    def _decode_inputs(self, r):
        """A decode plan's side of the seam: the buffers the full plan's neck and embed GEMM write, here inputs the caller fills."""
        self.feat_s0, self.feat_s1 = self.buf(r.f0, r.f0, 32, zero=True), self.buf(r.f1, r.f1, 64, zero=True)
        emb = self.buf(r.fs, r.fs, 256, F32, zero=True) if r.prompted else None
        self._decoder(r, emb, None if r.prompted else self._bufd(r.fs, r.fs, 256, F32, zero=True))

    # ---- one Hiera block ---------------------------------------------------------------------------------
    def _block(self, i, r, x, H, W, stats_in):
        """Emits block i's launches as r (hiera_route.BlockRoute) routes them.  stats_in: the statistics tensor the previous block left behind.
        -> (x, the statistics tensor left for the next block's norm1)"""
        wt, B, tl = self.wt, self.B, self.wt.tl
        dim, dout, heads, _, q_pool = wt.blocks[i]
        gam, bet = wt.ln[f"b{i}.norm1"]
        ln1 = (gam, bet, 1e-6)
        if r.stats_in is None:
            stats_in = None                                        # (none written for exactly these rows)
        parts = r.stats_in or 0
        if r.norm1 == "padded":
            # the padded grid is a zero-initialised buffer whose valid region the LayerNorm writes
            xn = self.buf(r.Hp, r.Wp, dim, tag="xn_padded", zero=True)
            op_layernorm(self.plan, f"b{i}.norm1", x.view(), gam, bet, xn.view(), 1e-6, pad=(H, W, r.Hp, r.Wp))
        elif r.norm1:
            xn = self.buf(H, W, dim, tag="xn")
            op_layernorm(self.plan, f"b{i}.norm1", x.view(), gam, bet, xn.view(), 1e-6)
        short = x if r.dimproj is None else self.buf(H // 2, W // 2, dout, F32)
        if r.dimproj == "tok_pool":
            op_tok_linear_pool(self.plan, f"b{i}.dimproj_pool", tl[f"b{i}.dimproj"], x.view(), short.view(), ln1, stats_in=stats_in if parts == 0 else None)
        elif r.dimproj:
            pj = self.buf(H, W, dout, F32, tag="dimproj")
            self.gemm(f"b{i}.dimproj", f"b{i}.dimproj", xn.view(), pj.view(), out_hw=(H, W) if r.padded else None)
            op_maxpool2(self.plan, f"b{i}.pool", pj.view(), short.view())
        qkv = None if r.qkv == "fused" else self.buf(r.Hp, r.Wp, 3 * dout, tag="qkv")
        if r.qkv == "tok":
            op_tok_linear(self.plan, f"b{i}.qkv", tl[f"b{i}.qkv"], x.view(), qkv.view(), ln=ln1, stats_in=stats_in, stats_parts=parts)
        elif r.qkv == "gemm":
            self.gemm(f"b{i}.qkv", f"b{i}.qkv", xn.view(), qkv.view())
        OH, OW = r.OH, r.OW
        ao = self.buf(*((r.Hp // 2, r.Wp // 2) if q_pool else (r.Hp, r.Wp)), dout, tag="ao")
        fl = 4 * r.nwin * heads * r.nq * r.nk * (dout // heads)
        if r.qkv == "fused":
            # the qkv tensor is neither written nor read back: the attention launch projects x itself
            pq, xv, rows = tl[f"b{i}.qkv_attn"], x.view(), B * H * W
            desc = self._attn_desc(i, r, ao, None, proj_x=xv.ptr, proj_ld=xv.ld, proj_K=dim, proj_w=pq.w.data_ptr(), proj_gamma=gam.data_ptr(),
                                   proj_beta=bet.data_ptr(), proj_eps=1e-6, proj_stats=stats_in.data_ptr() if stats_in is not None else None)
            op_attention(self.plan, f"b{i}.attn", desc, (x, ao, pq, gam, bet, stats_in), bytes_=rows * dim * 4 + ao.nbytes,
                         flops=2 * rows * 3 * dout * dim + fl, kind="attn_window")
        else:
            op_attention(self.plan, f"b{i}.attn", self._attn_desc(i, r, ao, qkv), (qkv, ao), bytes_=qkv.nbytes + ao.nbytes, flops=fl,
                         kind="attn_global" if r.attn == "global" else "attn_window")
        # x = shortcut + proj(attn)   (in place on the f32 residual stream); "fused": the prologue of the MLP launch below (proj_mlp.hpp), x1 is
        # neither written nor read back
        stats_fc1 = None if r.stats_fc1 is None else torch.empty(B * OH * OW, max(r.stats_fc1, 1), 2, dtype=torch.float32, device=self.dev)
        if r.proj == "tok":
            op_tok_linear(self.plan, f"b{i}.proj", tl[f"b{i}.proj"], ao.view(), short.view(), residual=True, stats_out=stats_fc1, stats_eps=1e-6)
        elif r.proj == "gemm":
            self.gemm(f"b{i}.proj", f"b{i}.proj", ao.view(), short.view(), res=short.view(), out_hw=(OH, OW) if r.padded else None)
        x = short               # (after a stage's last block the next one writes its own shortcut buffer, so x stays intact as the stage output)
        gam, bet = wt.ln[f"b{i}.norm2"]
        stats_out = None
        if r.mlp == "fused":
            if r.stats_mlp:
                stats_out = torch.empty(B * OH * OW, 2, dtype=torch.float32, device=self.dev)      # the next block's norm1 reads x once
            op_hiera_mlp(self.plan, f"b{i}.mlp", wt.mlp[f"b{i}"], x.view(), gam, bet, 1e-6, stats_out=stats_out, stats_eps=1e-6,
                         proj=(wt.mlp[f"b{i}.projmlp"], ao.view()) if r.proj == "fused" else None)
            return x, stats_out
        hid = self.buf(OH, OW, 4 * dout, tag="hid")
        if r.mlp == "tok_fc1":                                     # norm2 fused into fc1 (+ GELU)
            op_tok_linear(self.plan, f"b{i}.fc1", tl[f"b{i}.fc1"], x.view(), hid.view(), ln=(gam, bet, 1e-6), act=ACT_GELU, stats_in=stats_fc1,
                          stats_parts=r.stats_fc1 or 0)
        else:
            xn2 = self.buf(OH, OW, dout, tag="xn")
            op_layernorm(self.plan, f"b{i}.norm2", x.view(), gam, bet, xn2.view(), 1e-6)
            self.gemm(f"b{i}.fc1", f"b{i}.fc1", xn2.view(), hid.view(), act=ACT_GELU)
        if r.stats_fc2 is not None:
            stats_out = torch.empty(B * OH * OW, r.stats_fc2, 2, dtype=torch.float32, device=self.dev)
        self.gemm(f"b{i}.fc2", f"b{i}.fc2", hid.view(), x.view(), res=x.view(), row_stats=stats_out)
        return x, stats_out

    def _attn_desc(self, i, r, ao, qkv, **proj):
        """Descriptor of block i's attention over the qkv buffer, or (qkv None, proj = the proj_* fields) projecting inside the launch."""
        _, dout, heads, ws, q_pool = self.wt.blocks[i]
        hd, C3, step = dout // heads, 3 * dout, dout * ESIZE[self.dt]
        q, k, v = (None,) * 3 if qkv is None else (qkv.t.data_ptr() + j * step for j in range(3))
        sb = 0 if ws else r.nk                                     # windows are found through (win, grid); a global block strides image by image
        return make_attn_desc(q=q, k=k, v=v, o=ao.t.data_ptr(), q_sb=sb * C3, q_sh=hd, q_st=C3, k_sb=sb * C3, k_sh=hd, k_st=C3, v_sb=sb * C3, v_sh=hd, v_st=C3,
                              o_sb=sb * dout, o_sh=hd, o_st=dout, B=r.nwin, heads=heads, Nq=r.nq, Nk=r.nk, dqk=hd, dv=hd, scale=hd ** -0.5, dtype=self.dt,
                              win=ws, grid_h=r.Hp if ws else 0, grid_w=r.Wp if ws else 0, q_pool=1 if q_pool else 0, av_fp8=self.av_fp8,
                              q_log2=1 if r.q_log2 else 0, **proj)

    # ---- neck + mask decoder + tail: emits what self.droute (decoder_route.DecoderRoute) says ----------------------------------
    def _neck_decoder(self, st):
        """Up to `embed` (route.neck_launches()), then -- unless this is an encode plan -- everything behind it (route.decoder_launches())."""
        r = self.droute
        self.feat_s0, self.feat_s1, s2, s3 = self._neck(st, r)
        emb, keys = self._embed(r, s2, s3, "embed", "box" if r.prompted else "dense")
        if self.stage == "encode":                     # the route is the learned-prompt one; the prompted form follows it
            self.emb, self.keys0 = (self._embed(r, s2, s3, "embed_box", "box")[0] if self.wt.prompt_ok else None), keys
            return
        self._decoder(r, emb, keys)

    def _decoder(self, r, emb, keys):
        """emb: a prompted plan's per-image embedding, keys: the `dense` stream as the embed GEMM wrote it (the other is None)."""
        self.emb = emb
        # pairs: the image of pair n is pair_image[n]; the launches that derive it as n / P in a prompts = P plan take the table instead
        self.pair_image = torch.zeros(r.NB, dtype=torch.int32, device=self.dev) if self.pairs else None
        pm = _PairMap(self.P, self.pair_image)
        keys, kn = self._image_stream(r, pm, emb, keys)
        qn0, pe = self._tokens(r)
        # the two f32 residual streams -- tokens q (layer 0 REPLACES it, so it needs no init) and image `keys` -- with their operand-dtype copies
        s = SimpleNamespace(q=Buf(r.NB, 1, r.T, 256, F32, self.dev, zero=True), qn=self._bufd(1, r.T, 256, tag="qn"), emb=emb, keys=keys, kn=kn)
        for l in (0, 1):
            self._two_way_layer(l, r, s, qn0, pe, pm)
        self._t2i("final", r.castk[2], s, pe, pm)
        self._ln("norm_final", s.q, s.q)
        self.keys0, self.keys_out, self.tokens_out = keys, keys, s.q
        self._upscale_and_heads(r, s, pm)
        self._tail(r)

    def _bufd(self, *a, **k):                  # a buffer with the decoder's batch (pairs), where `buf` has the images'
        return self.buf(*a, batch=self.droute.NB, **k)

    def _G(self, name, src, dst, **kw):
        self.gemm(name, name, src, dst, kind="decoder", **kw)

    def _ln(self, name, src, dst, dst2=None, eps=1e-5, act=ACT_NONE):
        gam, bet = self.wt.ln[name]
        op_layernorm(self.plan, name, src.view(), gam, bet, dst.view(), eps, act=act, dst2=dst2.view() if dst2 is not None else None)

    def _attention(self, label, qb, q_off, kb, k_off, vb, v_off, ob, Nq, Nk, hd, q_map=_PER_PAIR, kv_map=_PER_PAIR):
        """q_map / kv_map: the _PairMap through which batch entry n finds its q / its k and v, where those are per IMAGE."""
        dt, NB, es, (q_bdiv, q_bmap), (kv_bdiv, kv_bmap) = self.dt, self.droute.NB, ESIZE[self.dt], q_map, kv_map
        desc = make_attn_desc(q=qb.t.data_ptr() + q_off * es, k=kb.t.data_ptr() + k_off * es, v=vb.t.data_ptr() + v_off * es, o=ob.t.data_ptr(),
                              q_sb=Nq * qb.C, q_sh=hd, q_st=qb.C, k_sb=Nk * kb.C, k_sh=hd, k_st=kb.C, v_sb=Nk * vb.C, v_sh=hd, v_st=vb.C,
                              o_sb=Nq * ob.C, o_sh=hd, o_st=ob.C, B=NB, heads=8, Nq=Nq, Nk=Nk, dqk=hd, dv=hd, scale=hd ** -0.5, dtype=dt,
                              win=0, grid_h=0, grid_w=0, q_pool=0, q_bdiv=q_bdiv, kv_bdiv=kv_bdiv,
                              q_bmap=q_bmap.data_ptr() if q_bmap is not None else None, kv_bmap=kv_bmap.data_ptr() if kv_bmap is not None else None)
        op_attention(self.plan, label, desc, (qb, kb, vb, ob, q_bmap, kv_bmap), flops=4 * NB * 8 * Nq * Nk * hd, kind="decoder")

    def _neck(self, st, r):
        """FPN levels 0 / 1 from the first two stage outputs, and the last two as GEMM operands -> (feat_s0, feat_s1, s2, s3)."""
        def cast(j):                       # GEMM operands in compute dtype (stage outputs are f32 residual streams)
            if j not in r.casts:
                return st[j]
            o = self.buf(st[j].H, st[j].W, st[j].C, self.dt)
            op_cast(self.plan, f"cast.s{j}", st[j].view(), o.view())
            return o
        feats = (self.buf(r.f0, r.f0, 32), self.buf(r.f1, r.f1, 64))
        for j, (key, dst) in enumerate(zip(("feat_s0", "feat_s1"), feats)):
            if r.neck[j] == "tok":
                op_tok_linear(self.plan, key, self.wt.tl[key], st[j].view(), dst.view(), ln="cast", kind="neck")     # reads the f32 stage output itself
            else:
                self.gemm(key, key, cast(j).view(), dst.view(), kind="neck")
        return feats + (cast(2), cast(3))

    def _embed(self, r, s2, s3, label, form):
        """FPN level 2, the seam between an encode and a decode plan -> (emb, keys), one of them None.  form "dense": + the learned dense prompt,
        straight into the decoder's image stream `keys`; "box": + no_mem_embed + no_mask_embed (both in the GEMM bias), per image, `emb`."""
        srcs = [(s2.view(), 0), (s3.view(), 1)]
        if form == "dense":
            keys = self._bufd(r.fs, r.fs, 256, F32)
            self.gemm(label, "embed", srcs, keys.view(), res=_ConstView(self.wt.const["dense"], 256), res_mod=r.fs * r.fs, kind="neck")
            return None, keys
        emb = self.buf(r.fs, r.fs, 256, F32)
        self.gemm(label, "embed_box", srcs, emb.view(), kind="neck")
        return emb, None

    def _image_stream(self, r, pm, emb, keys):
        """The launch r.stream names behind `embed` -> (keys: the decoder's per-pair f32 image stream, kn: its copy in the operand dtype --
        allocated here, once; r.castk says which launches write it)."""
        wt, dt, B, NB, lib, fs, f0, P = self.wt, self.dt, self.B, r.NB, _lib.load(), r.fs, r.f0, r.fs * r.fs
        kn = self._bufd(fs, fs, 256, tag="kn")
        if r.stream == "dense":            # the embed GEMM wrote the stream itself
            return keys, kn
        keys = self._bufd(fs, fs, 256, F32)
        # the launch that makes the per-pair stream of emb ("shared": none, see DecoderRoute.stream); in a 16-bit plan it writes the operand copy too
        kn16, copy16 = ((kn.t.data_ptr(), dt), NB * P * 256 * 2) if is16(dt) else ((None, F16), 0)
        if r.stream == "mask_prompt":      # keys = emb + mask_downscaling(mask_in) - no_mask_embed
            self.mask_in = torch.zeros(NB, f0, f0, dtype=torch.float32, device=self.dev)
            head = (self.mask_in.data_ptr(), emb.t.data_ptr(), wt.const["mask_down"].data_ptr(), keys.t.data_ptr()) + kn16
            fn, tail = (lib.cvmi_mask_prompt_embed_pairs, (NB, pm.table.data_ptr(), fs)) if self.pairs else (lib.cvmi_mask_prompt_embed, (B, pm.rep, fs))
            op_call(self.plan, "mask_prompt_embed", "decoder", fn, head + tail, keep=(emb, keys, kn, pm.table),
                    bytes_=NB * f0 * f0 * 4 + (B + NB) * P * 256 * 4 + copy16, flops=2 * NB * P * (16 * 4 + 16 * 16 + 256 * 16))
        elif r.stream == "gather":
            op_call(self.plan, "gather_embed", "decoder", lib.cvmi_gather_images,
                    (emb.t.data_ptr(), keys.t.data_ptr()) + kn16 + (P * 256 * 4, pm.table.data_ptr(), NB),
                    keep=(emb, keys, kn, pm.table), bytes_=2 * NB * P * 256 * 4 + copy16)
        elif r.stream == "repeat":
            op_call(self.plan, "repeat_embed", "decoder", lib.cvmi_repeat_images, (emb.t.data_ptr(), keys.t.data_ptr(), P * 256 * 4, B, pm.rep),
                    keep=(emb, keys), bytes_=(B + NB) * P * 256 * 4)
        return keys, kn

    def _tokens(self, r):
        """-> (the tokens layer 0 reads, in the operand dtype; pe(name, C): the residual arguments that add (token PE) @ W^T of constant `name`, C
        wide, to a GEMM on the tokens: a constant of the checkpoint's own tokens, or a column group of the prompt tokens' `token_pe` GEMM)."""
        wt, dt, NB, T = self.wt, self.dt, r.NB, r.T
        qn0 = Buf(NB, 1, T, 256, dt, self.dev)
        if r.tokens == "const":
            qn0.t.copy_(wt.const["tokens"].to(TORCH_DTYPE[dt]).view(1, 1, T, 256).expand(NB, 1, T, 256))
            return qn0, lambda name, C_: dict(res=_ConstView(wt.const[name], C_), res_mod=T)
        self.coords = torch.zeros(NB, self.K, 2, dtype=torch.float32, device=self.dev)
        self.labels = torch.full((NB, self.K), -1, dtype=torch.int32, device=self.dev)
        self.tokens0 = tok0 = Buf(NB, 1, T, 256, F32, self.dev)
        op_call(self.plan, "prompt_tokens", "decoder", _lib.load().cvmi_prompt_tokens,
                (self.coords.data_ptr(), self.labels.data_ptr(), wt.const["gauss"].data_ptr(), wt.const["out_tokens"].data_ptr(),
                 wt.const["prompt_table"].data_ptr(), float(wt.image_size), tok0.t.data_ptr(), qn0.t.data_ptr(), dt, NB, self.K, 6),
                keep=(tok0, qn0), bytes_=NB * T * 256 * 6)
        pe_all = Buf(NB, 1, T, wt.pc["token_pe"].N, dt, self.dev)
        self._G("token_pe", qn0.view(), pe_all.view())
        return qn0, lambda name, C_: dict(res=pe_all.view(wt.pe_off[name][0], C_))

    def _t2i(self, p, castk, s, pe, pm):
        """Tokens attend to the image (layer 0, layer 1, `final`) -> the image stream's operand copy it read.  castk (the route's) "emb": layer 0 of a
        shared plan, the image-side tensors are per IMAGE, made from the embedding."""
        T, fs, shared = self.droute.T, self.droute.fs, castk == "emb"
        op_cast(self.plan, f"{p}.castq", s.q.view(), s.qn.view())
        kn = self.buf(fs, fs, 256, tag="kn_shared") if shared else s.kn
        if castk:
            op_cast(self.plan, f"{p}.castk", (s.emb if shared else s.keys).view(), kn.view())
        tq = self._bufd(1, T, 128, tag="t2i_q")
        self._G(f"{p}.q", s.qn.view(), tq.view(), **pe(f"{p}.q_pe", 128))
        kv = self.buf(fs, fs, 256, tag="t2i_kv_shared") if shared else self._bufd(fs, fs, 256, tag="t2i_kv")
        self._G(f"{p}.kv", kn.view(), kv.view(), res=_ConstView(self.wt.const[f"{p}.kv_pe"], 256), res_mod=fs * fs)
        ao = self._bufd(1, T, 128, tag="t2i_ao")
        self._attention(f"{p}.attn", tq, 0, kv, 0, kv, 128, ao, T, fs * fs, 16, kv_map=pm if shared else _PER_PAIR)
        self._G(f"{p}.out", ao.view(), s.q.view(), res=s.q.view())
        return kn

    def _two_way_layer(self, l, r, s, qn0, pe, pm):
        T, fs, p, q, qn, keys, shared = r.T, r.fs, f"l{l}", s.q, s.qn, s.keys, r.castk[l] == "emb"      # shared: layer 0's image-side tensors are per IMAGE
        # --- self attention on the tokens
        qkv = self._bufd(1, T, 768, tag="sa_qkv")
        if l:              # (layer 0 reads the initial tokens as they are, without a positional residual)
            op_cast(self.plan, f"{p}.sa.cast", q.view(), qn.view())
        self._G(f"{p}.sa.qkv", (qn if l else qn0).view(), qkv.view(), **(pe(f"{p}.sa.qkv_pe", 768) if l else {}))
        ao = self._bufd(1, T, 256, tag="sa_ao")
        self._attention(f"{p}.sa.attn", qkv, 0, qkv, 256, qkv, 512, ao, T, T, 32)
        self._G(f"{p}.sa.out", ao.view(), q.view(), res=q.view() if l else None)         # layer 0: queries REPLACED (skip_first_layer_pe)
        self._ln(f"{p}.norm1", q, q)
        # --- tokens attend to the image
        kn = self._t2i(f"{p}.t2i", r.castk[l], s, pe, pm)
        self._ln(f"{p}.norm2", q, q)
        # --- MLP on the tokens
        op_cast(self.plan, f"{p}.mlp.cast", q.view(), qn.view())
        hid = self._bufd(1, T, 2048, tag="mlp_hid")
        self._G(f"{p}.mlp1", qn.view(), hid.view(), act=ACT_RELU)
        self._G(f"{p}.mlp2", hid.view(), q.view(), res=q.view())
        self._ln(f"{p}.norm3", q, q)
        # --- image attends to the tokens
        op_cast(self.plan, f"{p}.i2t.castq", q.view(), qn.view())
        iq = self.buf(fs, fs, 128, tag="i2t_q_shared") if shared else self._bufd(fs, fs, 128, tag="i2t_q")
        self._G(f"{p}.i2t.q", kn.view(), iq.view(), res=_ConstView(self.wt.const[f"{p}.i2t.q_pe"], 128), res_mod=fs * fs)
        ikv = self._bufd(1, T, 256, tag="i2t_kv")
        self._G(f"{p}.i2t.kv", qn.view(), ikv.view(), **pe(f"{p}.i2t.kv_pe", 256))
        ao3 = self._bufd(fs, fs, 128, tag="i2t_ao")
        self._attention(f"{p}.i2t.attn", iq, 0, ikv, 0, ikv, 128, ao3, fs * fs, T, 16, q_map=pm if shared else _PER_PAIR)
        # shared: the first write of the per-pair image stream, keys[n] = emb[image of pair n] + out-projection
        res = dict(res=s.emb.view(), res_mod=fs * fs, res_rep=pm.rep, res_map=pm.table) if shared else dict(res=keys.view())
        self._G(f"{p}.i2t.out", ao3.view(), keys.view(), **res)
        self._ln(f"{p}.norm4", keys, keys, dst2=s.kn if is16(self.dt) else None)      # + the 16-bit copy the next k / v projection reads (no cast pass)

    def _mlp3(self, name, src, dst, act=ACT_NONE):             # a three-layer head `name`.0 - .2 on one row per pair
        h1, h2 = self._bufd(1, 1, 256, tag="h1"), self._bufd(1, 1, 256, tag="h2")
        self._G(f"{name}.0", src, h1.view(), act=ACT_RELU)
        self._G(f"{name}.1", h1.view(), h2.view(), act=ACT_RELU)
        self._G(f"{name}.2", h2.view(), dst, act=act)

    def _upscale_and_heads(self, r, s, pm):
        dt, NB, T = self.dt, r.NB, r.T
        # --- upscaling: act1(ln1(dc1(src) + s1)) ; act2(dc2(.) + s0), s1 / s0 of the pair's image
        u1 = self._bufd(r.f1, r.f1, 64)
        self._G("up1", s.kn.view(), u1.view(), res=self.feat_s1.view(), shuffle_cout=64, res_rep=pm.rep, res_map=pm.table)
        self._ln("up_ln", u1, u1, eps=1e-6, act=ACT_GELU)
        self.up = u2 = self._bufd(r.f0, r.f0, 32)
        self._G("up2", u1.view(), u2.view(), res=self.feat_s0.view(), shuffle_cout=32, act=ACT_GELU, act_after_res=True, res_rep=pm.rep, res_map=pm.table)
        # --- hypernetwork MLPs on the 4 mask tokens, IoU head on the iou token (rows strided by T*256)
        op_cast(self.plan, "heads.cast", s.q.view(), s.qn.view())
        token = lambda i: _RowsView(s.qn.t, NB, 256, ld=T * 256, offset=i * 256, dtype=dt)
        self.hyper, self.iou4 = Buf(NB, 1, 4, 32, F32, self.dev), Buf(NB, 1, 1, 4, F32, self.dev)
        for i in range(4):
            self._mlp3(f"hyper{i}", token(2 + i), _RowsView(self.hyper.t, NB, 32, ld=128, offset=i * 32, dtype=F32))
        self._mlp3("iou", token(1), self.iou4.view(), act=ACT_SIGMOID)

    def _tail(self, r):                        # masks, dynamic multimask selection, upsample + refinement
        wt, dt, NB, R, f0, lib = self.wt, self.dt, r.NB, self.wt.image_size, r.f0, _lib.load()
        P0, NM = f0 * f0, 3 if r.masks == "multimask_out" else 1                  # NM: masks returned per pair
        self.masks4 = torch.empty(NB, 4, f0, f0, dtype=torch.float32, device=self.dev)
        self.areas = torch.zeros(NB, 2, dtype=torch.int32, device=self.dev)
        self.low_res = torch.empty(NB, NM, f0, f0, dtype=torch.float32, device=self.dev)
        self.iou = torch.empty(NB, NM, dtype=torch.float32, device=self.dev)
        self.sel = torch.zeros(NB, dtype=torch.int32, device=self.dev)
        op_call(self.plan, "hyper_masks", "tail", lib.cvmi_hyper_masks,
                (self.hyper.t.data_ptr(), 32, self.up.t.data_ptr(), 32, dt, 32, self.masks4.data_ptr(), self.areas.data_ptr(), NB, P0, 0.05),
                keep=(self.hyper, self.up), bytes_=NB * P0 * (32 * ESIZE[dt] + 16), flops=2 * NB * P0 * 128)
        if r.masks == "multimask_out":
            op_call(self.plan, "multimask_out", "tail", lib.cvmi_multimask_out,
                    (self.masks4.data_ptr(), self.iou4.t.data_ptr(), 4, self.low_res.data_ptr(), self.iou.data_ptr(), NB, P0), bytes_=NB * P0 * 24)
        else:
            op_call(self.plan, "select_mask", "tail", lib.cvmi_select_mask,
                    (self.masks4.data_ptr(), self.areas.data_ptr(), self.iou4.t.data_ptr(), 4, 1 if self.dynamic else 0, 0.98, self.low_res.data_ptr(),
                     self.iou.data_ptr(), self.sel.data_ptr(), NB, P0), bytes_=NB * P0 * 8)
        self.high_res = torch.empty(NB, NM, R, R, dtype=torch.float32, device=self.dev) if r.upsample else None
        if r.upsample == "upsample_refine":            # the refinement head belongs to the learned-prompt wrapper (sam2_infer.py:269-270)
            ks = (ctypes.c_int * len(wt.kernels))(*wt.kernels)
            taps = sum(k * k for k in wt.kernels)
            op_call(self.plan, "upsample_refine", "tail", lib.cvmi_upsample_refine,
                    (self.low_res.data_ptr(), NB, f0, f0, self.high_res.data_ptr(), R, R, wt.refine_params.data_ptr(), ks, len(wt.kernels), 4),
                    keep=(ks,), bytes_=NB * (P0 + R * R) * 4, flops=2 * NB * R * R * 4 * taps)
        elif r.upsample:
            op_call(self.plan, "upsample", "tail", lib.cvmi_bilinear_f32,
                    (self.low_res.data_ptr(), NB * NM, f0, f0, self.high_res.data_ptr(), R, R, None, 0.0), bytes_=NB * NM * (P0 + R * R) * 4)


class _ConstView:
    """Constant [rows, C] device tensor posing as a residual View (ptr, ld)."""

    def __init__(self, t, C):
        self.t, self.c = t, C

    ptr = property(lambda s: s.t.data_ptr())
    ld = property(lambda s: s.c)


class _RowsView:
    """Strided row matrix posing as a [B,1,1,C] conv source / destination."""

    def __init__(self, t, rows, C, ld, offset, dtype):
        self.t, self.B, self.H, self.W, self.c, self._ld, self.off, self.dtype = t, rows, 1, 1, C, ld, offset, dtype

    ptr = property(lambda s: s.t.data_ptr() + s.off * s.t.element_size())
    ld = property(lambda s: s._ld)
