"""Which launches a SAM 2 plan takes after the Hiera trunk -- FPN neck, prompt handling, two-way transformer, upscaling, heads, tail -- decided apart
from emitting them, in the manner of hiera_route.py: `route_decoder` is a pure function of shapes, dtype, prompt mode and switches (no device, no
buffers), tested without a GPU (tests/test_decoder_route_cpu.py).  `sam2.Sam2Plan._neck_decoder` emits what the `DecoderRoute` says."""
from typing import NamedTuple, Optional

from ._lib import F32
from .engine import is16, tok_linear_supported
from .hiera_route import SamSwitches

STREAM_LAUNCH = dict(repeat="repeat_embed", gather="gather_embed", mask_prompt="mask_prompt_embed")      # the one launch a stream adds behind `embed`


class DecoderRoute(NamedTuple):
    NB: int                       # decoder batch: images (learned prompts), or (image, prompt) pairs
    T: int                        # tokens per batch entry
    f0: int                       # grids: masks and FPN level 0 (image_size / 4),
    f1: int                       # FPN level 1,
    fs: int                       # the decoder's image stream (image_size / 16)
    prompted: bool
    neck: tuple                   # per FPN level (feat_s0, feat_s1): "tok" (tok_linear reads the f32 stage output itself) | "gemm" (tiled GEMM)
    casts: tuple                  # the stage outputs that get a `cast.s{j}` launch (the GEMM operands of a 16-bit plan)
    # where the per-pair image stream `keys` comes from:
    #   "dense"        learned prompts: embed adds the learned dense prompt and writes it
    #   "shared"       no launch: until layer 0's image -> token attention writes into it, the stream of every prompt of an image IS that image's
    #                  embedding, so layer 0 reads the B per-image copies (k / v and q projections on B images, not B * P; the attention kernels index
    #                  the shared batch entry; i2t.out's residual add broadcasts and is the first write of the per-pair stream).  16-bit plans only:
    #                  f32 parity mode keeps the literal repeat_image formulation (upstream MaskDecoder.predict_masks) as the cross-check
    #   "repeat"       the embedding of image n / P, copied          "gather"   ... of image pair_image[n], copied
    #   "mask_prompt"  the embedding + mask_downscaling(mask_in): differs per pair from the start
    stream: str
    # what the `castk` launch of (l0.t2i, l1.t2i, final) converts into the image stream's operand copy: "emb" (per image) | "keys" | None = no launch,
    # a 16-bit plan's copy is already written: layer 0's by gather_embed / mask_prompt_embed, layer 1's and final's by the norm4 before them
    castk: tuple
    tokens: str                   # "const": the checkpoint's tokens, positional residuals folded into constants | "prompt": prompt_tokens + token_pe
    masks: str                    # "multimask_out" | "select_mask"
    upsample: Optional[str]       # "upsample_refine" | "upsample" | None: no high-res output

    def launches(self):
        """[(label, kind)] in launch order.  A second statement of the order in which `Sam2Plan._neck_decoder` emits, kept for the tests: the
        fixture test derives sequences from it without a GPU, and tests/test_decoder_route_gpu.py holds the emitter to it -- change the two
        together."""
        return self.neck_launches() + self.decoder_launches()

    def neck_launches(self):
        """The launches up to and including `embed` -- behind the trunk they end an encode plan (`Sam2Plan(stage="encode")`, which adds the other
        form of the embed GEMM); what `embed` writes is the seam: the predictor's image embedding."""
        cast = lambda *names: [(n, "cast") for n in names]
        out = []
        for j in (0, 1):
            out += cast(*([f"cast.s{j}"] if j in self.casts else [])) + [(f"feat_s{j}", "neck")]
        return out + cast(*(f"cast.s{j}" for j in (2, 3) if j in self.casts)) + [("embed", "neck")]

    def decoder_launches(self):
        """Everything behind `embed`: all of a decode plan (`Sam2Plan(stage="decode")`)."""
        d = lambda *names: [(n, "decoder") for n in names]
        cast = lambda *names: [(n, "cast") for n in names]
        ln = lambda *names: [(n, "layernorm") for n in names]
        t2i = lambda p, castk: cast(f"{p}.castq", *([f"{p}.castk"] if castk else [])) + d(f"{p}.q", f"{p}.kv", f"{p}.attn", f"{p}.out")
        out = d(*([STREAM_LAUNCH[self.stream]] if self.stream in STREAM_LAUNCH else []), *(["prompt_tokens", "token_pe"] if self.tokens == "prompt" else []))
        for l in (0, 1):
            p = f"l{l}"
            out += cast(*([f"{p}.sa.cast"] if l else [])) + d(f"{p}.sa.qkv", f"{p}.sa.attn", f"{p}.sa.out") + ln(f"{p}.norm1")
            out += t2i(f"{p}.t2i", self.castk[l]) + ln(f"{p}.norm2")
            out += cast(f"{p}.mlp.cast") + d(f"{p}.mlp1", f"{p}.mlp2") + ln(f"{p}.norm3")
            out += cast(f"{p}.i2t.castq") + d(f"{p}.i2t.q", f"{p}.i2t.kv", f"{p}.i2t.attn", f"{p}.i2t.out") + ln(f"{p}.norm4")
        out += t2i("final", self.castk[2]) + ln("norm_final")
        out += d("up1") + ln("up_ln") + d("up2") + cast("heads.cast")
        out += d(*(f"{h}.{j}" for h in ("hyper0", "hyper1", "hyper2", "hyper3", "iou") for j in range(3)))
        return out + [(n, "tail") for n in ("hyper_masks", self.masks, self.upsample) if n]


def route_decoder(dtype, B, image_size, sw: SamSwitches, prompts=0, pairs=0, points=3, mask_prompt=False, multimask=False, high_res=True, refine=True,
                  neck_tok=(False, False), stage_dims=(), n_tok=38):
    """Route of everything after the trunk.  refine: the weights carry the refinement head; neck_tok: feat_s0 / feat_s1 have a token-stationary
    packing; stage_dims: widths of the stage outputs; n_tok: the checkpoint's own tokens (learned-prompt plans); sw: the plan's switches."""
    if pairs and prompts:
        raise ValueError("pairs (a pair-to-image table) and prompts (P per image) are alternatives")
    if pairs < 0 or pairs > 65535:
        raise ValueError("pairs must be in 1 .. 65535")
    prompted = bool(prompts or pairs)
    if (mask_prompt or multimask) and not prompted:
        raise ValueError("mask_prompt / multimask need prompts > 0 (the learned-prompt wrapper always runs single-mask without a mask input)")
    dual, f0 = is16(dtype), image_size // 4
    # the stage outputs are f32 residual streams, stage j on the (f0 >> j)^2 grid; tok_linear takes whole 256-row workgroups
    neck = tuple("tok" if sw.neckcast and neck_tok[j] and tok_linear_supported(stage_dims[j], dtype, B * (f0 >> j) ** 2) else "gemm" for j in (0, 1))
    casts = () if dtype == F32 else tuple(j for j in (0, 1) if neck[j] == "gemm") + (2, 3)
    stream = "dense" if not prompted else "mask_prompt" if mask_prompt else "shared" if dual and sw.share_l0 else "gather" if pairs else "repeat"
    castk0 = "emb" if stream == "shared" else None if dual and stream in ("gather", "mask_prompt") else "keys"
    return DecoderRoute(
        NB=int(pairs) or (B * prompts if prompts else B), T=6 + points if prompted else n_tok, f0=f0, f1=f0 // 2, fs=f0 // 4, prompted=prompted,
        neck=neck, casts=casts, stream=stream, castk=(castk0,) + ((None,) if dual else ("keys",)) * 2, tokens="prompt" if prompted else "const",
        masks="multimask_out" if multimask else "select_mask",
        upsample=None if not high_res else "upsample_refine" if refine and not prompted else "upsample")
