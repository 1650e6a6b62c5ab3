"""Reference for mask prompts and multimask output (`infer_masks(mask_input=..., multimask_output=...)`, csrc/mask_prompt.hip), plain torch.

`mask_downscaling` restates upstream `PromptEncoder.mask_downscaling` (mask_in_chans = 16) from a state dict with the upstream key names;
tests/test_mask_prompt_cpu.py checks it against `transformers`' Sam2MaskEmbedding and a by-hand known answer.  `mask_prompt_keys` is what
`cvmi_mask_prompt_embed` computes; `predict_prompts_masked` is upstream `SAM2ImagePredictor._predict` with `mask_input` / `multimask_output`,
built from the oracle's own modules (oracle/sam2_model.py restates the prompt encoder without the mask stack, so the stack comes from here)."""
import torch
import torch.nn.functional as F

from oracle import sam2_model as osam

MD = "sam_prompt_encoder.mask_downscaling"
NO_MASK = "sam_prompt_encoder.no_mask_embed.weight"
SHAPES = {f"{MD}.0.weight": (4, 1, 2, 2), f"{MD}.0.bias": (4,), f"{MD}.1.weight": (4,), f"{MD}.1.bias": (4,),
          f"{MD}.3.weight": (16, 4, 2, 2), f"{MD}.3.bias": (16,), f"{MD}.4.weight": (16,), f"{MD}.4.bias": (16,),
          f"{MD}.6.weight": (256, 16, 1, 1), f"{MD}.6.bias": (256,)}
# wrong implementations the op comparison must tell from the right one (test_mask_prompt_cpu.py)
MUTANTS = ("taps1", "taps2", "unbiased", "keep_no_mask", "pair_major")


def _ln2d(x, w, b, unbiased=False):
    """LayerNorm2d: per pixel over the channels, biased variance, eps 1e-6 inside the root."""
    u = x.mean(1, keepdim=True)
    d = x - u
    s = d.pow(2).sum(1, keepdim=True) / (x.shape[1] - (1 if unbiased else 0))
    return w[None, :, None, None] * (d / torch.sqrt(s + 1e-6)) + b[None, :, None, None]


def mask_downscaling(sd, mask, dtype=torch.float64, mutant=None):
    """mask [n, 1, 4 fs, 4 fs] logits -> dense [n, 256, fs, fs], evaluated in `dtype`."""
    t = {k: sd[k].to(dtype) for k in SHAPES}
    w1, w2 = t[f"{MD}.0.weight"], t[f"{MD}.3.weight"]
    if mutant == "taps1":
        w1 = w1.transpose(2, 3)
    if mutant == "taps2":
        w2 = w2.transpose(2, 3)
    x = F.conv2d(mask.to(dtype), w1, t[f"{MD}.0.bias"], stride=2)
    x = F.gelu(_ln2d(x, t[f"{MD}.1.weight"], t[f"{MD}.1.bias"], mutant == "unbiased"))
    x = F.conv2d(x, w2, t[f"{MD}.3.bias"], stride=2)
    x = F.gelu(_ln2d(x, t[f"{MD}.4.weight"], t[f"{MD}.4.bias"], mutant == "unbiased"))
    return F.conv2d(x, t[f"{MD}.6.weight"], t[f"{MD}.6.bias"])


def mask_prompt_keys(sd, mask, emb, rep, dtype=torch.float64, mutant=None):
    """cvmi_mask_prompt_embed: mask [B*rep, 4 fs, 4 fs], emb [B, fs*fs, 256] (its bias already holds no_mask_embed) ->
    keys [B*rep, fs*fs, 256] = emb[i // rep] + mask_downscaling(mask[i]) - no_mask_embed; pairs are image-major."""
    n, B = mask.shape[0], emb.shape[0]
    dense = mask_downscaling(sd, mask[:, None], dtype, mutant).flatten(2).transpose(1, 2)
    image = torch.arange(n) % B if mutant == "pair_major" else torch.arange(n) // rep
    keys = emb.to(dtype)[image] + dense
    return keys if mutant == "keep_no_mask" else keys - sd[NO_MASK].to(dtype).reshape(1, 1, 256)


def pack_params(sd):
    """The parameter vector of cvmi_mask_prompt_embed (include/cvmi355.h), packed independently of Sam2Weights."""
    parts = [sd[k].float().reshape(-1) for k in SHAPES]
    parts[-1] = parts[-1] - sd[NO_MASK].float().reshape(-1)
    return torch.cat(parts)


def op_state_dict(params):
    """What the op reference reads, from a `SamSyntheticParams` alone (no packed model): the mask stack and no_mask_embed."""
    return {**params.mask_prompt_state_dict(), NO_MASK: params.tensor(NO_MASK, (1, 256), "unit")}


# (B, rep, fs) of the op test: a partial wave; the image-major broadcast; an odd size with a tail in every group; the production geometry;
# and 3200 groups of 64 pixels for a grid capped at 768 workgroups of 4 waves -- some workgroups go through their loop twice
OP_SHAPES = ((1, 1, 5), (2, 3, 16), (3, 2, 9), (1, 2, 64), (2, 25, 64))


def op_inputs(B, rep, fs, sd, seed=0):
    """Inputs of the op test: logits 6 randn, one all-zero plane and one plane of +-30 checkerboard (with fewer than three planes: the first /
    last third of the output rows of the first / last plane instead, so that random logits remain); emb = 0.1 randn + no_mask_embed (what
    the embed GEMM hands over, so that the output is of the size of the image embedding plus the dense prompt)."""
    g = torch.Generator().manual_seed(1000 * seed + 100 * B + 10 * rep + fs)
    n = B * rep
    mask = 6 * torch.randn(n, 4 * fs, 4 * fs, generator=g)
    yy, xx = torch.meshgrid(torch.arange(4 * fs), torch.arange(4 * fs), indexing="ij")
    checker = 30.0 * (1 - 2 * ((yy + xx) % 2)).float()
    rows = 4 * fs if n >= 3 else 4 * (fs // 3)
    mask[0, :rows] = 0
    mask[n - 1, 4 * fs - rows:] = checker[4 * fs - rows:]
    emb = 0.1 * torch.randn(B, fs * fs, 256, generator=g) + sd[NO_MASK].float().reshape(1, 1, 256)
    return mask, emb


def _encode(wrapper, images):
    m = wrapper.sam2_model
    embed, high_res = wrapper.encode(images)
    embed = embed + m.no_mem_embed.view(1, -1, 1, 1)
    fs = embed.shape[-1]
    return embed, high_res, osam.dense_pe(m.sam_prompt_encoder.pe_layer.positional_encoding_gaussian_matrix, fs, fs), fs


def _sparse(m, b, boxes, points, labels):
    cs, ls = [], []
    if boxes is not None:
        cs.append(boxes[b].float().reshape(-1, 2, 2))
        ls.append(torch.tensor([[2, 3]], dtype=torch.long).expand(boxes.shape[1], 2))
    if points is not None:
        cs.append(points[b].float())
        ls.append(labels[b].long())
    return m.sam_prompt_encoder.embed_points(torch.cat(cs, 1), torch.cat(ls, 1), pad=True)


def predict_prompts_masked(wrapper, sd, images, boxes=None, points=None, labels=None, mask_input=None, multimask_output=False, margins=False):
    """Upstream predictor semantics with a mask prompt: per image, image_embed = FPN level 2 + no_mem_embed, sparse = corners, clicks, one
    padding point, dense = mask_downscaling(mask_input[b]) [P,256,fs,fs] (no_mask_embed when mask_input is None), decoder with
    repeat_image=True.  -> (high_res [B,P,n,R,R], low_res [B,P,n,R/4,R/4], iou [B,P,n]) with n = 3 for multimask_output, else 1.
    margins=True: also (stability [B,P] of token 0, iou4 [B,P,4]) -- what the single-mask selection decides on."""
    m = wrapper.sam2_model
    embed, high_res, pe, fs = _encode(wrapper, images)
    his, lows, ious, stabs, iou4s = [], [], [], [], []
    for b in range(images.shape[0]):
        sparse = _sparse(m, b, boxes, points, labels)
        dense = m.sam_prompt_encoder.dense_no_mask(fs) if mask_input is None else mask_downscaling(sd, mask_input[b][:, None].float(), torch.float32)
        hr = [h[b:b + 1] for h in high_res]
        low, iou, _ = m.sam_mask_decoder(embed[b:b + 1], pe, sparse, dense, hr, multimask_output=multimask_output, repeat_image=True)
        his.append(F.interpolate(low, size=(m.image_size, m.image_size), mode="bilinear", align_corners=False))
        lows.append(low); ious.append(iou)
        if margins:
            masks4, iou4, _ = m.sam_mask_decoder.predict_masks(embed[b:b + 1], pe, sparse, dense, hr, repeat_image=True)
            flat = masks4[:, 0].flatten(1)
            ai, au = (flat > m.sam_mask_decoder.delta).sum(-1).float(), (flat > -m.sam_mask_decoder.delta).sum(-1).float()
            stabs.append(torch.where(au > 0, ai / au, torch.ones_like(au))); iou4s.append(iou4)
    out = (torch.stack(his), torch.stack(lows), torch.stack(ious))
    return out + (torch.stack(stabs), torch.stack(iou4s)) if margins else out


def selection_is_clear(stab, iou4, thresh=0.98):
    """The precondition of a single-mask comparison: no pair's stability score within 0.01 of the threshold, and its two best multimask IoU
    predictions at least 1e-2 apart -- otherwise a selection flipped by rounding would pose as an error of the masks."""
    top = iou4[..., 1:].sort(-1, descending=True).values
    return bool(((stab - thresh).abs() >= 0.01).all()) and bool(((top[..., 0] - top[..., 1]) >= 1e-2).all())


# input seeds of the mini-model GPU tests (weights: seed 9, std 0.05): on the reference every pair of every prompt kind selects clearly with
# MINI_SEED, the box prompts of REPLAY_SEED too (`selection_is_clear`; checked on the CPU by tests/test_mask_prompt_cpu.py)
MINI_SEED, REPLAY_SEED = 28, 11


def mini_inputs(seed, R=256, B=2, P=3):
    """Inputs of the mini-model tests: images, boxes (xyxy, sides U(24, 200) scaled to R / 1024), two clicks per prompt (foreground,
    background) and a mask prompt of 6 randn logits."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 3, R, R, generator=g)
    side = (24 + 176 * torch.rand(B, P, 2, generator=g)) * (R / 1024)
    xy = torch.rand(B, P, 2, generator=g) * (R - side)
    pts = torch.rand(B, P, 2, 2, generator=g) * (R - 1)
    lab = torch.tensor([1, 0]).expand(B, P, 2).clone()
    mask = 6 * torch.randn(B, P, R // 4, R // 4, generator=g)
    return dict(x=x, boxes=torch.cat((xy, xy + side), -1), points=pts, labels=lab, mask=mask)
