"""Drop-in for the names the reference imports from its `src/sam2_infer.py`
(`from .sam2_infer import SAM2Transforms, get_modified_sam2, device`, circuit_analyzer.py:17-21),
backed by the cvmi355 HIP kernels.  See SURVEY.md 8(b) for the exact surface the callers rely on.
"""
import itertools
import os
import threading
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib
from ._lib import BF16, F16, F32
from .engine import TORCH_DTYPE, require_gpu
from .sam2 import HIERA_L, Sam2Plan, Sam2Weights, SamBaseCheckpointParams, SamStateDictParams, SamSyntheticParams

# the reference picks its device at import time (sam2_infer.py:19-25); on PyTorch-ROCm "cuda" is the MI355X
device = torch.device("cuda") if torch.cuda.is_available() else torch.device("cpu")


def _hiera_from_yaml(path):
    """Trunk hyper-parameters from a sam2 Hydra YAML (models/configs/sam2.1_hiera_l.yaml:9-16, :89)."""
    import yaml
    with open(path) as f:
        cfg = yaml.safe_load(f)
    m = cfg["model"]
    t = m["image_encoder"]["trunk"]
    hiera = dict(embed_dim=t.get("embed_dim", 96), num_heads=t.get("num_heads", 1), stages=tuple(t.get("stages", (2, 3, 16, 3))),
                 global_att_blocks=tuple(t.get("global_att_blocks", (12, 16, 20))), window_spec=tuple(t.get("window_spec", (8, 4, 14, 7))))
    return hiera, int(m.get("image_size", 1024))


def _is_list(a):
    return isinstance(a, (list, tuple))


def pack_prompt_lists(B, R, boxes=None, points=None, point_labels=None, mask_input=None, pair_bucket=32):
    """The host half of `infer_masks` with one prompt list per image (no GPU needed): boxes = B tensors [P_b, 4], points / point_labels = B
    tensors [P_b, K, 2] / [P_b, K] (one K for all), mask_input = B float tensors [P_b, R/4, R/4]; P_b may be 0.  -> a dict of host tensors
    for a `Sam2Plan(pairs=cap)`:
      sizes [P_0 .. P_{B-1}], N = their sum, cap = N rounded up to a multiple of pair_bucket, K = tokens per prompt (box corners, clicks, the
      closing padding point), coords f32 [cap, K, 2], labels i32 [cap, K], pair_image i32 [cap] (pair n belongs to image pair_image[n];
      pairs are image-major), mask f32 [cap, R/4, R/4] or None.
    Slots N .. cap - 1 are padding: image 0, the box [0, 0, R, R] (without boxes: not-a-point tokens only) and a zero mask.
    Raises ValueError for a list of the wrong length, entries that are not tensors or have the wrong shape, counts that differ between the
    arguments, and N == 0."""
    f0 = R // 4
    if pair_bucket < 1:
        raise ValueError("pair_bucket must be >= 1")
    if boxes is None and points is None:
        raise ValueError("prompt lists need boxes and / or points")
    if points is not None and point_labels is None:
        raise ValueError("points need point_labels")
    given = dict(boxes=boxes, points=points, point_labels=point_labels if points is not None else None, mask_input=mask_input)
    for name, a in given.items():
        if a is None:
            continue
        if not _is_list(a):
            raise ValueError(f"{name}: with one prompt list per image every prompt argument is a list of B = {B} tensors")
        if len(a) != B:
            raise ValueError(f"{name}: {len(a)} entries for B = {B} images")
        if not all(torch.is_tensor(t) for t in a):
            raise ValueError(f"{name}: every entry must be a tensor (an image without prompts: an empty one, e.g. torch.zeros(0, 4))")
    sizes = [int(t.shape[0]) if t.dim() > 0 else -1 for t in (boxes if boxes is not None else points)]
    nk = 0
    if boxes is not None:
        for b, t in enumerate(boxes):
            if t.dim() != 2 or t.shape[1] != 4:
                raise ValueError(f"boxes[{b}] must be [P_b, 4] xyxy, got {tuple(t.shape)}")
    if points is not None:
        ks = {int(t.shape[1]) for t in points if t.dim() == 3}
        if len(ks) != 1 or 0 in ks:
            raise ValueError("points: one click count K > 0 for every prompt of every image ([P_b, K, 2]; label -1 pads a shorter list)")
        nk = ks.pop()
        for b, (t, l) in enumerate(zip(points, point_labels)):
            if t.dim() != 3 or t.shape[2] != 2 or tuple(l.shape) != tuple(t.shape[:2]):
                raise ValueError(f"points[{b}] must be [P_b, K, 2] with point_labels[{b}] [P_b, K], got {tuple(t.shape)} / {tuple(l.shape)}")
            if t.shape[0] != sizes[b]:
                raise ValueError(f"image {b}: {sizes[b]} boxes but {t.shape[0]} point prompts")
            if l.numel() and (int(l.min()) < -1 or int(l.max()) > 1):
                raise ValueError("point_labels must be -1 (padding token), 0 (background) or 1 (foreground)")
    if mask_input is not None:
        for b, t in enumerate(mask_input):
            if not t.is_floating_point() or tuple(t.shape) != (sizes[b], f0, f0):
                raise ValueError(f"mask_input[{b}] must be float [P_b={sizes[b]}, {f0}, {f0}] low-res logits, got {t.dtype} {tuple(t.shape)}")
    N = sum(sizes)
    if N == 0:
        raise ValueError("no prompt in any image (N = 0): nothing to segment")
    cap = -(-N // pair_bucket) * pair_bucket
    nb = 2 if boxes is not None else 0
    K = nb + nk + 1                                            # + the closing padding point
    coords = torch.zeros(cap, K, 2, dtype=torch.float32)
    labels = torch.full((cap, K), -1, dtype=torch.int32)
    pair_image = torch.zeros(cap, dtype=torch.int32)
    pair_image[:N] = torch.repeat_interleave(torch.arange(B, dtype=torch.int32), torch.tensor(sizes))
    if boxes is not None:
        coords[:N, :2] = torch.cat([t.detach().float().cpu().reshape(-1, 2, 2) for t in boxes])
        coords[N:, 1] = float(R)                               # padding: the whole-image box [0, 0, R, R]
        labels[:, 0], labels[:, 1] = 2, 3
    if points is not None:
        coords[:N, nb:nb + nk] = torch.cat([t.detach().float().cpu() for t in points])
        labels[:N, nb:nb + nk] = torch.cat([l.detach().cpu().to(torch.int32) for l in point_labels])
    if int(pair_image.min()) < 0 or int(pair_image.max()) >= B:            # the kernels read the table unchecked (include/cvmi355.h)
        raise ValueError("pair_image outside [0, B)")
    return dict(sizes=sizes, N=N, cap=cap, K=K, coords=coords, labels=labels, pair_image=pair_image, has_mask=mask_input is not None)


M2M_MAX_PAIRS = 65535                            # cvmi_m2m_fanout: the pair is the second dimension of its grid
_WEIGHTS_IDS = itertools.count(1)                # identity of one packing of weights (`SAM2Model.load_params`), unique in the process


class Sam2Embeddings:
    """What `SAM2Model.encode_images` returns and `infer_masks` takes in the place of images (upstream's set_image / predict split): the tensors
    at the seam between the encoder and the mask decoder, owned by the caller --
      feat_s0 [B, R/4, R/4, 32], feat_s1 [B, R/8, R/8, 64] in the model's dtype (FPN levels 0 / 1 behind conv_s0 / conv_s1),
      emb   f32 [B, R/16, R/16, 256]: the image embedding box / click / mask prompts decode from (None: a checkpoint without a prompt encoder),
      dense f32 [B, R/16, R/16, 256]: the same plus the learned dense prompt, the learned-prompt decode's image stream
    -- with image_size, dtype (the CVMI dtype of the model) and weights_id, the identity of the packed weights that made them.  A plain container
    that works on tensors of any device: `len()`, `nbytes`, `e[i]` / `e[a:b]` / `e[[i, j]]` (a new Sam2Embeddings; an int keeps the batch
    axis) and `Sam2Embeddings.cat` build batches out of cached images."""
    TENSORS = ("feat_s0", "feat_s1", "emb", "dense")

    def __init__(self, feat_s0, feat_s1, emb, dense, image_size, dtype, weights_id):
        self.feat_s0, self.feat_s1, self.emb, self.dense = feat_s0, feat_s1, emb, dense
        self.image_size, self.dtype, self.weights_id = int(image_size), dtype, weights_id
        f0, fs = self.image_size // 4, self.image_size // 16
        B = feat_s0.shape[0]
        want = dict(feat_s0=(B, f0, f0, 32), feat_s1=(B, f0 // 2, f0 // 2, 64), emb=(B, fs, fs, 256), dense=(B, fs, fs, 256))
        for name, t in self.tensors():
            if tuple(t.shape) != want[name]:
                raise ValueError(f"Sam2Embeddings.{name}: shape {tuple(t.shape)}, expected {want[name]}")

    def tensors(self):
        return [(n, getattr(self, n)) for n in self.TENSORS if getattr(self, n) is not None]

    def signature(self):
        """What two embeddings must share to be batched together or decoded by a model."""
        return (self.weights_id, self.dtype, self.image_size, self.emb is not None)

    def __len__(self):
        return int(self.feat_s0.shape[0])

    @property
    def device(self):
        return self.feat_s0.device

    @property
    def nbytes(self):
        return sum(t.numel() * t.element_size() for _, t in self.tensors())

    def _like(self, fn):
        return Sam2Embeddings(*(fn(getattr(self, n)) if getattr(self, n) is not None else None for n in self.TENSORS),
                              self.image_size, self.dtype, self.weights_id)

    def __getitem__(self, idx):
        if isinstance(idx, bool) or not isinstance(idx, (int, slice, list, tuple)):
            raise TypeError("Sam2Embeddings index: an int, a slice or a list of ints")
        B = len(self)
        if isinstance(idx, int):
            if not -B <= idx < B:
                raise IndexError(f"image {idx} of {B}")
            idx = slice(idx % B, idx % B + 1)
        if isinstance(idx, slice):
            return self._like(lambda t: t[idx])
        rows = [int(i) for i in idx]
        if any(not -B <= i < B for i in rows):
            raise IndexError(f"images {rows} of {B}")
        return self._like(lambda t: t[torch.tensor(rows, dtype=torch.long, device=t.device)])

    @staticmethod
    def cat(parts):
        parts = list(parts)
        if not parts:
            raise ValueError("Sam2Embeddings.cat of an empty list")
        if any(not isinstance(e, Sam2Embeddings) for e in parts):
            raise TypeError("Sam2Embeddings.cat takes Sam2Embeddings")
        if any(e.signature() != parts[0].signature() for e in parts[1:]):
            raise ValueError("Sam2Embeddings.cat: embeddings of different weights, dtypes or image sizes do not mix")
        first = parts[0]
        return Sam2Embeddings(*(torch.cat([getattr(e, n) for e in parts]) if getattr(first, n) is not None else None for n in first.TENSORS),
                              first.image_size, first.dtype, first.weights_id)


class SAM2Model:
    """What `get_modified_sam2(...)` returns: `.load_state_dict`, `.eval`, `.sam2_model.image_size`,
    `__call__(x) -> (high_res, low_res, iou)` (sam2_infer.py:220-275), plus `infer_masks`."""

    def __init__(self, hiera=HIERA_L, image_size=1024, dtype="f16", dev="cuda", use_refinement=True, refinement_kernels=(3, 5, 7, 11),
                 embedding_r=4, lora_rank=4, lora_alpha=16, dynamic_multimask_via_stability=True, attn="16"):
        """attn="fp8": the softmax(QK^T) V products of Hiera's 256-key windows and global blocks on the block-scaled fp8 MFMA (BASELINE configs[4];
        off by default: it is slower than the 16-bit product on this path -- DESIGN.md section 5 -- and costs ~3 mantissa bits on V)."""
        require_gpu()
        self.attn = attn
        self.hiera, self.image_size = hiera, image_size
        self.dtype = {"f16": F16, "fp16": F16, "f32": F32, "fp32": F32, "bf16": BF16}[dtype] if isinstance(dtype, str) else dtype
        self.dev = dev
        self.cfg = dict(use_refinement=use_refinement, refinement_kernels=tuple(refinement_kernels), embedding_r=embedding_r)
        self.lora = (lora_rank, lora_alpha)
        self.dynamic = dynamic_multimask_via_stability
        self.sam2_model = SimpleNamespace(image_size=image_size)          # circuit_analyzer.py:237-240 reads .sam2_model.image_size
        self.weights, self.params, self._pending, self.weights_id = None, None, None, 0
        self.stream = torch.cuda.Stream(device=dev)
        self._slot_streams = {0: self.stream}                               # plan slot -> stream (slot 1: a second plan instance on its own stream, so
        self._plans = {}                                                    # that two independent batches run side by side: CircuitPipeline)
        self._lock = threading.Lock()                                       # one analyzer is shared across sessions (app.py:134)
        self.training = False
        self.pair_bucket = 32                                               # prompt lists: the pair count is rounded up to a multiple (bounds the plans / graphs)

    # -- nn.Module-like surface the reference touches
    def load_params(self, params):
        self.params, self._pending = params, None
        with torch.cuda.device(self.dev):
            self.weights = Sam2Weights(params, self.hiera, self.image_size, self.dtype, self.dev, **self.cfg)
        self.weights_id = next(_WEIGHTS_IDS)                  # embeddings of an earlier packing are refused (`Sam2Embeddings.weights_id`)
        self._plans.clear()
        return self

    def load_state_dict(self, sd, strict=True):
        if "state_dict" in sd and not torch.is_tensor(sd["state_dict"]):
            sd = sd["state_dict"]
        return self.load_params(SamStateDictParams(sd, *self.lora))

    def eval(self):
        self.training = False
        return self

    def to(self, *_a, **_k):
        return self

    def slot_stream(self, slot):
        if slot not in self._slot_streams:
            self._slot_streams[slot] = torch.cuda.Stream(device=self.dev)
        return self._slot_streams[slot]

    def _packed_weights(self):
        if self.weights is None and self._pending is not None:
            self.load_params(self._pending)           # base checkpoint only (no fine-tuned state dict followed): pack it now
        if self.weights is None:
            raise RuntimeError("SAM2 weights not loaded (call load_state_dict first)")
        return self.weights

    def plan(self, B, prompts=0, high_res=True, points=3, slot=0, mask_prompt=False, multimask=False, pairs=0, stage="full"):
        """pairs = cap: the plan of `cap` (image, prompt) pairs with a pair-to-image table (prompt lists); keyed on cap, not on the pair count.
        stage: "full", or one side of the encode / decode split (`Sam2Plan`); the key of a full plan carries no stage."""
        wt = self._packed_weights()
        key = (B, prompts, high_res, points if (prompts or pairs) else 0, slot, bool(mask_prompt), bool(multimask), pairs) + ((stage,) if stage != "full" else ())
        if key not in self._plans:
            with torch.cuda.device(self.dev):
                self._plans[key] = Sam2Plan(wt, B, self.slot_stream(slot), self.dynamic, prompts=prompts, points=points, high_res=high_res, attn=self.attn,
                                            mask_prompt=mask_prompt, multimask=multimask, pairs=pairs, stage=stage)
        return self._plans[key]

    def _stage_images(self, p, images):
        """Checked copy of a [B,3,R,R] tensor into the plan's NHWC input buffer.  Runs inside `torch.cuda.stream(self.stream)`; the caller's
        stream has been made a predecessor (`wait_stream`), so device inputs produced there are complete when the copy reads them."""
        lib = _lib.load()
        B = images.shape[0]
        x = images.to(self.dev)
        if x.dtype not in (torch.float32, torch.float16, torch.bfloat16) or (x.dtype == torch.float16) != (self.dtype == F16) and x.dtype != torch.float32:
            x = x.float()                                     # (a 16-bit input of the OTHER 16-bit type goes through f32)
        src_dt = {torch.float32: F32, torch.float16: F16, torch.bfloat16: BF16}[x.dtype]
        sp = self.stream.cuda_stream
        if x.permute(0, 2, 3, 1).is_contiguous():            # already channels-last memory (SAM2Transforms output)
            _lib.check(lib.cvmi_cast(x.data_ptr(), 3, src_dt, p.x_in.t.data_ptr(), 3, self.dtype, B * self.image_size ** 2, 3, sp), "cast")
        else:
            x = x.contiguous()
            _lib.check(lib.cvmi_nchw_to_nhwc(x.data_ptr(), src_dt, p.x_in.t.data_ptr(), self.dtype, 3, B, 3, self.image_size, self.image_size, sp), "nchw_to_nhwc")
        return x                                              # keep alive until the stream has consumed it

    @staticmethod
    def _stage_embeddings(p, e):
        """D2D copies of embeddings into a decode plan's input buffers, on the model's stream like `_stage_images`."""
        p.feat_s0.t.copy_(e.feat_s0, non_blocking=True)
        p.feat_s1.t.copy_(e.feat_s1, non_blocking=True)
        if p.droute.prompted:
            p.emb.t.copy_(e.emb, non_blocking=True)
        else:
            p.keys0.t.copy_(e.dense, non_blocking=True)      # the decoder updates its image stream in place: staged before every run

    def _seam(self, p):
        """The seam tensors of an encode plan as (un-owned) embeddings."""
        return Sam2Embeddings(p.feat_s0.t, p.feat_s1.t, p.emb.t if p.emb is not None else None, p.keys0.t, self.image_size, self.dtype, self.weights_id)

    def _run(self, p, src, outs, before=None, refine=(), pairs=0, m2m=None):
        """Stage -> replay the plan -> copy `outs` = [(plan tensor, fresh tensor)] -- all on the model's stream, which first waits for the
        caller's current stream and is synchronised before returning (the reference's call is synchronous).  The output copies are
        part of the stream's order, so the next caller's replay (another session thread, app.py:134) cannot overwrite the plan's
        buffers under them.
        src: images for a full plan, or `Sam2Embeddings` for a decode plan (copied into its inputs first, then `before`).
        refine: the decode plans of the mask-feedback passes that follow p (itself a decode plan then; with images the encode plan runs in
        front, once): each gets the embeddings and p's prompts, and `mask_in` from its predecessor's low_res / iou through
        cvmi_best_candidate over the `pairs` real pairs, launched on the stream between the two replays.
        m2m = (q, clamp): the mask-to-mask pass instead -- q, the single-mask decode plan of NM * pairs pairs, gets the embeddings, and
        cvmi_m2m_fanout writes its mask_in / coords / labels / pair_image from p's low_res and p's prompts, between the two replays."""
        lib, sp = _lib.load(), self.stream.cuda_stream
        chain = tuple(refine) + ((m2m[0],) if m2m is not None else ())
        self.stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(self.stream):
            keep, e = src, src if isinstance(src, Sam2Embeddings) else None
            if e is not None or chain:
                for q in (p,) + chain:
                    if q.plan.graph is None:                  # capture's warm pass runs on the buffers as they are: in front of the staging
                        q.plan.capture()
            if e is None and chain:
                enc = self.plan(src.shape[0], stage="encode")
                keep = self._stage_images(enc, src)
                enc.plan.run()
                e = self._seam(enc)
            if e is not None:
                self._stage_embeddings(p, e)
            if before is not None:
                before()
            if e is None:
                keep = self._stage_images(p, src)
            p.plan.run()
            prev, fed = p, {id(p)}
            for q in refine:
                if id(q) not in fed:                          # inputs no replay writes: once per plan
                    fed.add(id(q))
                    self._stage_embeddings(q, e)
                    q.coords.copy_(p.coords, non_blocking=True)
                    q.labels.copy_(p.labels, non_blocking=True)
                    if q.pair_image is not None:
                        q.pair_image.copy_(p.pair_image, non_blocking=True)
                NM, f0 = prev.low_res.shape[1], prev.low_res.shape[2]
                _lib.check(lib.cvmi_best_candidate(prev.low_res.data_ptr(), prev.iou.data_ptr(), NM, q.mask_in.data_ptr(), None, pairs, f0 * f0, sp), "best_candidate")
                q.mask_in[pairs:].zero_()                     # the padding rows of a pairs = cap plan
                q.plan.run()
                prev = q
            if m2m is not None:
                q, clamp = m2m
                self._stage_embeddings(q, e)
                NM, f0, n2 = p.low_res.shape[1], p.low_res.shape[2], p.low_res.shape[1] * pairs
                tables = (p.pair_image, q.pair_image) if p.pair_image is not None else (None, None)
                _lib.check(lib.cvmi_m2m_fanout(p.low_res.data_ptr(), NM, clamp, q.mask_in.data_ptr(), p.coords.data_ptr(), p.labels.data_ptr(),
                                               tables[0].data_ptr() if tables[0] is not None else None, q.coords.data_ptr(), q.labels.data_ptr(),
                                               tables[1].data_ptr() if tables[1] is not None else None, pairs, f0 * f0, p.coords.shape[1], sp), "m2m_fanout")
                if n2 < q.mask_in.shape[0]:                   # the padding rows of a pairs = cap plan: a zero mask, not-a-point tokens, image 0
                    q.mask_in[n2:].zero_()
                    q.coords[n2:].zero_()
                    q.labels[n2:].fill_(-1)
                    q.pair_image[n2:].zero_()
                q.plan.run()
            for a, b in outs:
                b.copy_(a, non_blocking=True)
        self.stream.synchronize()
        del keep

    def _check_images(self, images):
        if not (torch.is_tensor(images) and images.dim() == 4 and images.shape[1] == 3 and images.shape[2] == images.shape[3] == self.image_size):
            raise ValueError(f"expected a [B,3,{self.image_size},{self.image_size}] tensor")

    def _check_src(self, src):
        """images [B,3,R,R] or the `Sam2Embeddings` of this model's weights -> B."""
        if not isinstance(src, Sam2Embeddings):
            self._check_images(src)
            return src.shape[0]
        self._packed_weights()
        if src.signature()[:3] != (self.weights_id, self.dtype, self.image_size):
            raise ValueError("these embeddings were made by other weights, another dtype or another image size (encode_images of THIS model)")
        if len(src) == 0 or any(not t.is_cuda for _, t in src.tensors()):
            raise ValueError("embeddings to decode must be a non-empty batch on the device")
        return len(src)

    def encode_images(self, images):
        """upstream `SAM2ImagePredictor.set_image`: images [B,3,R,R] (as `infer_masks` takes them) -> `Sam2Embeddings`, which `infer_masks`
        accepts in the place of images, any number of times, with any prompts: only the mask decoder runs then (bit for bit what the one-shot
        call computes).  The tensors are the caller's; the model keeps nothing of them."""
        self._check_images(images)
        with self._lock, torch.cuda.device(self.dev):
            p = self.plan(images.shape[0], stage="encode")
            seam = self._seam(p)
            out = seam._like(torch.empty_like)                                        # the caller's tensors, as in __call__
            self._run(p, images, [(a, getattr(out, n)) for n, a in seam.tensors()])
            return out

    def __call__(self, images, points=None, point_labels=None, masks_prompt=None, multimask_output=False):
        B = self._check_src(images)
        if multimask_output:
            raise NotImplementedError("the wrapper always runs multimask_output=False (sam2_infer.py:257)")
        with self._lock, torch.cuda.device(self.dev):
            p = self.plan(B, stage="decode" if isinstance(images, Sam2Embeddings) else "full")
            out = [torch.empty_like(t) for t in (p.high_res, p.low_res, p.iou)]       # the caller's tensors (its allocator pool, not the model stream's)
            self._run(p, images, list(zip((p.high_res, p.low_res, p.iou), out)))
            return tuple(out)

    forward = __call__

    def infer_masks(self, images, boxes=None, return_high_res=True, points=None, point_labels=None, mask_input=None, multimask_output=False,
                    refine_steps=0, m2m=False, m2m_clamp=32.0):
        """Batched segmentation entry point (north_star).  images [B,3,R,R], or the `Sam2Embeddings` `encode_images` made of them (the trunk
        and the neck are then not run again: every prompt form below decodes from them, with the same checks and the same results).
        No prompt: exactly `SAM2ImageWrapper.forward` (learned prompts) -> (high_res [B,1,R,R], low_res [B,1,R/4,R/4], iou [B,1]).
        boxes [B,P,4] (xyxy in the R x R input pixel space, e.g. detector boxes scaled by R / original size) and / or
        points [B,P,K,2] (x, y) with point_labels [B,P,K] (1 foreground click, 0 background click, -1 "not a point" padding token,
        upstream's filler for ragged click lists -- still a token the decoder sees): upstream
        SAM2ImagePredictor prompting on the same weights -- a box enters as two corner points labelled 2 / 3, clicks follow it,
        one padding point closes the list -- one mask per prompt (multimask_output=False with the stability fallback) ->
        (high_res logits [B,P,R,R] or None, low_res logits [B,P,R/4,R/4] (unclamped), iou [B,P]).
        mask_input [B,P,R/4,R/4] (float, host or device; needs boxes and / or points): upstream's mask prompt -- low-res logits, e.g. the
        low_res of an earlier call, enter through `sam_prompt_encoder.mask_downscaling` as the dense prompt in the place of no_mask_embed.
        multimask_output=True (needs a prompt): the three multimask candidates in token order with their predicted IoUs, no stability
        fallback -> (high_res [B,P,3,R,R] or None, low_res [B,P,3,R/4,R/4], iou [B,P,3]).
        Prompt lists: boxes a list of B tensors [P_b,4], points / point_labels lists of [P_b,K,2] / [P_b,K], mask_input a list of
        [P_b,R/4,R/4] -- every image its own number of prompts, 0 included; all lists given agree on B and on every P_b.  The decoder runs on
        the N = sum P_b pairs (rounded up to a multiple of `pair_bucket`), nothing is padded per image.  Lists in, lists out: high_res,
        low_res and iou are each a list of B tensors ([P_b,R,R], [P_b,R/4,R/4], [P_b]; a candidate axis of 3 after P_b with
        multimask_output=True), `torch.split` views of one packed [N,...] allocation.
        refine_steps = k > 0 (needs a prompt and a checkpoint with mask_downscaling): upstream's recipe for ambiguous prompts on the device.
        The call as given is pass 1; k single-mask passes on the same prompts follow, each with the previous pass's best candidate (the
        highest predicted IoU, cvmi_best_candidate) as its mask prompt.  The trunk runs once, nothing goes through the host, and the
        last pass's (high_res or None, low_res, iou) come back in the single-mask shapes, whatever multimask_output was.
        m2m=True (needs a prompt and a checkpoint with mask_downscaling; not together with refine_steps): the mask-to-mask pass of upstream's
        automatic mask generator (use_m2m).  The call as given is pass 1 and yields NM candidates per prompt (3 with multimask_output, else
        1); ONE single-mask pass follows in which EVERY candidate is a prompt of its own: the prompt it came from plus its low-res logits,
        clamped to [-m2m_clamp, m2m_clamp] as upstream's predictor returns them, as the mask prompt (cvmi_m2m_fanout).  The trunk runs once,
        nothing goes through the host, the stream is synchronised once.  -> the refined candidates in pass 1's shapes and candidate order:
        (high_res [B,P,NM,R,R] or None, low_res [B,P,NM,R/4,R/4], iou [B,P,NM]), without the NM axis when NM = 1; lists of [P_b,NM,...] in
        the list form.  At most 65535 (image, prompt) pairs per call.  m2m_clamp: upstream's bound is 32; the argument exists so that a
        test can make the clamp bite on a model whose logits never reach 32."""
        if not isinstance(refine_steps, int) or isinstance(refine_steps, bool) or refine_steps < 0:
            raise ValueError("refine_steps must be an int >= 0")
        m2m = self._check_m2m(m2m, m2m_clamp, refine_steps)
        if _is_list(boxes) or _is_list(points) or _is_list(point_labels) or _is_list(mask_input):
            return self._infer_masks_lists(images, boxes, return_high_res, points, point_labels, mask_input, multimask_output, refine_steps, m2m)
        if boxes is None and points is None:
            if mask_input is not None or refine_steps or m2m is not None:
                raise ValueError("mask_input / refine_steps / m2m need boxes and / or points (a mask-only prompt is not built)")
            return self(images, multimask_output=multimask_output)
        B = self._check_src(images)
        bx = pts = None
        if boxes is not None:
            bx = torch.as_tensor(boxes, dtype=torch.float32)
            if bx.dim() != 3 or bx.shape[0] != B or bx.shape[2] != 4 or bx.shape[1] == 0:
                raise ValueError(f"boxes must be [B={B}, P>0, 4] xyxy, got {tuple(bx.shape)}")
        if points is not None:
            pts = torch.as_tensor(points, dtype=torch.float32)
            if point_labels is None:
                raise ValueError("points need point_labels")
            lab = torch.as_tensor(point_labels).to(torch.int32)
            if pts.dim() != 4 or pts.shape[0] != B or pts.shape[3] != 2 or pts.shape[1] == 0 or pts.shape[2] == 0 or tuple(lab.shape) != tuple(pts.shape[:3]):
                raise ValueError(f"points must be [B={B}, P>0, K>0, 2] with point_labels [B, P, K], got {tuple(pts.shape)} / {tuple(lab.shape)}")
            if bx is not None and bx.shape[1] != pts.shape[1]:
                raise ValueError("boxes and points disagree on the number of prompts per image")
            if int(lab.min()) < -1 or int(lab.max()) > 1:
                raise ValueError("point_labels must be -1 (padding token), 0 (background) or 1 (foreground)")
        P = (bx if bx is not None else pts).shape[1]
        nb, nk = (2 if bx is not None else 0), (pts.shape[2] if pts is not None else 0)
        K = nb + nk + 1                                            # + the closing padding point
        f0 = self.image_size // 4
        mk = None
        if mask_input is not None:
            mk = torch.as_tensor(mask_input)
            if not mk.is_floating_point() or tuple(mk.shape) != (B, P, f0, f0):
                raise ValueError(f"mask_input must be float [B={B}, P={P}, {f0}, {f0}] low-res logits, got {mk.dtype} {tuple(mk.shape)}")
        coords = torch.zeros(B * P, K, 2, dtype=torch.float32)
        labels = torch.full((B * P, K), -1, dtype=torch.int32)
        if bx is not None:
            coords[:, :2] = bx.reshape(B * P, 2, 2)
            labels[:, 0], labels[:, 1] = 2, 3
        if pts is not None:
            coords[:, nb:nb + nk] = pts.reshape(B * P, nk, 2)
            labels[:, nb:nb + nk] = lab.reshape(B * P, nk)
        pk = dict(kw=dict(prompts=P), N=B * P, K=K, coords=coords, labels=labels, pair_image=None, mask=mk.reshape(B * P, f0, f0) if mk is not None else None)
        hi, lo, iou = self._prompt_passes(images, B, pk, return_high_res, multimask_output, refine_steps, m2m)
        return tuple(t.view(B, P, *t.shape[1:]) if t is not None else None for t in (hi, lo, iou))

    @staticmethod
    def _check_m2m(m2m, m2m_clamp, refine_steps):
        """-> the clamp bound as a float when the mask-to-mask pass is asked for, else None."""
        if not m2m:
            return None
        if refine_steps:
            raise ValueError("m2m=True and refine_steps > 0 do not combine: one of the two mask-feedback forms per call")
        clamp = float(m2m_clamp)
        if not clamp >= 0:
            raise ValueError("m2m_clamp must be a number >= 0")
        return clamp

    def _prompt_passes(self, src, B, pk, return_high_res, multimask_output, refine_steps, m2m=None):
        """The prompted decode of N (image, prompt) pairs packed on the host -- pk: kw = the plan's prompts=P or pairs=cap, N, K, coords, labels,
        pair_image (pairs plans), mask ([N, R/4, R/4], or a list of tensors that concatenate to it, or None) -- and the refine_steps mask-feedback
        passes behind it -> (high_res or None, low_res, iou) with N in front.  m2m = the clamp bound: the mask-to-mask pass behind it instead,
        a single-mask plan of NM * N pairs (prompts = NM * P, or pairs = NM * N rounded up to the bucket) -> the same with [N, NM] in front."""
        R, f0, N = self.image_size, self.image_size // 4, pk["N"]
        masked, multimask = pk["mask"] is not None, bool(multimask_output)
        if m2m is not None and N > M2M_MAX_PAIRS:
            raise ValueError(f"m2m=True with {N} (image, prompt) pairs: cvmi_m2m_fanout takes at most {M2M_MAX_PAIRS} per call")
        with self._lock, torch.cuda.device(self.dev):
            if (masked or refine_steps or m2m is not None) and not self._packed_weights().mask_prompt_ok:
                raise RuntimeError("this checkpoint carries no sam_prompt_encoder.mask_downscaling tensors: mask_input is unavailable")
            chained = bool(refine_steps) or m2m is not None
            stage = "decode" if chained or isinstance(src, Sam2Embeddings) else "full"            # one-shot use: one graph and no copies
            plan = lambda high_res, mask_prompt, multi: self.plan(B, high_res=high_res, points=pk["K"], mask_prompt=mask_prompt, multimask=multi, stage=stage,
                                                                  **pk["kw"])
            p = plan(return_high_res and not chained, masked, multimask)
            refine = [plan(return_high_res and i == refine_steps - 1, True, False) for i in range(refine_steps)]
            last, fan = (refine[-1] if refine else p), None
            if m2m is not None:
                NM = 3 if multimask else 1
                kw2 = dict(pairs=-(-NM * N // self.pair_bucket) * self.pair_bucket) if "pairs" in pk["kw"] else dict(prompts=NM * pk["kw"]["prompts"])
                last = self.plan(B, high_res=return_high_res, points=pk["K"], mask_prompt=True, multimask=False, stage="decode", **kw2)
                fan = (last, m2m)

            def prompts_in():                                          # on the model's stream, in front of the replay that reads them
                p.coords.copy_(pk["coords"], non_blocking=False)
                p.labels.copy_(pk["labels"], non_blocking=False)
                if pk["pair_image"] is not None:
                    p.pair_image.copy_(pk["pair_image"], non_blocking=False)
                if masked:
                    mask = pk["mask"]
                    p.mask_in[:N].copy_(torch.cat([t.detach().to(self.dev, torch.float32) for t in mask]) if _is_list(mask) else mask, non_blocking=False)
                    p.mask_in[N:].zero_()
            shp = (N, 3) if multimask and not refine else (N,)            # (the mask-to-mask pass keeps pass 1's candidate axis)
            lo, iou = torch.empty(*shp, f0, f0, dtype=torch.float32, device=self.dev), torch.empty(*shp, dtype=torch.float32, device=self.dev)
            hi = torch.empty(*shp, R, R, dtype=torch.float32, device=self.dev) if return_high_res else None
            rows = N * (3 if multimask and fan is not None else 1)       # of `last`: every candidate is a pair of the mask-to-mask plan
            outs = ([(last.low_res[:rows].view(*shp, f0, f0), lo), (last.iou[:rows].view(*shp), iou)]
                    + ([(last.high_res[:rows].view(*shp, R, R), hi)] if return_high_res else []))
            self._run(p, src, outs, before=prompts_in, refine=refine, pairs=N, m2m=fan)
            return hi, lo, iou

    def _infer_masks_lists(self, images, boxes, return_high_res, points, point_labels, mask_input, multimask_output, refine_steps=0, m2m=None):
        """`infer_masks` with one prompt list per image: pack on the host (`pack_prompt_lists`), replay the `pairs=cap` plan, split."""
        B = self._check_src(images)
        pk = pack_prompt_lists(B, self.image_size, boxes, points, point_labels, mask_input, self.pair_bucket)
        sizes = pk["sizes"]
        pk.update(kw=dict(pairs=pk["cap"]), mask=mask_input if pk["has_mask"] else None)
        hi, lo, iou = self._prompt_passes(images, B, pk, return_high_res, multimask_output, refine_steps, m2m)
        return (list(torch.split(hi, sizes)) if hi is not None else None), list(torch.split(lo, sizes)), list(torch.split(iou, sizes))


def get_modified_sam2(model_cfg_path, checkpoint_path, device="cuda", use_high_res_features=True, use_peft=True, lora_rank=12,
                      lora_alpha=16, lora_dropout=0.2, lora_target_modules=None, use_wrapper=True, trainable_embedding_r=4,
                      use_refinement_layer=False, refinement_kernels=(3, 5, 7, 11), kernel_channels=4, dtype="f16", attn="16", **_loss_and_optimizer_kwargs):
    """Same signature as sam2_infer.py:277-305 (loss / optimizer kwargs accepted and ignored).  `checkpoint_path`
    may be 'synthetic[:seed]' for seeded random weights; a real base checkpoint ({'model': state_dict}) is accepted
    but every tensor is expected to come from the fine-tuned state dict loaded afterwards (circuit_analyzer.py:227-233)."""
    if not use_wrapper or not use_high_res_features:
        raise NotImplementedError("only the reference configuration (use_wrapper=True, use_high_res_features=True) is built")
    hiera, image_size = HIERA_L, 1024
    if isinstance(model_cfg_path, str) and os.path.exists(model_cfg_path):
        hiera, image_size = _hiera_from_yaml(model_cfg_path)
    elif isinstance(model_cfg_path, str) and os.path.exists(model_cfg_path.lstrip("/")):
        hiera, image_size = _hiera_from_yaml(model_cfg_path.lstrip("/"))          # the reference prepends "/" for Hydra (circuit_analyzer.py:204)
    model = SAM2Model(hiera, image_size, dtype=dtype, dev=str(device), use_refinement=use_refinement_layer, refinement_kernels=refinement_kernels,
                      embedding_r=trainable_embedding_r, lora_rank=lora_rank, lora_alpha=lora_alpha, attn=attn)
    if isinstance(checkpoint_path, str) and checkpoint_path.startswith("synthetic"):
        seed = int(checkpoint_path.split(":")[1]) if ":" in checkpoint_path else 0
        targets = lora_target_modules if (use_peft and lora_target_modules is not None) else ()
        model.load_params(SamSyntheticParams(seed=seed, lora_targets=targets, r=lora_rank, alpha=lora_alpha))
    elif isinstance(checkpoint_path, str) and os.path.exists(checkpoint_path):
        # The reference always loads the fine-tuned state dict next (circuit_analyzer.py:227-233), which replaces every tensor:
        # packing the base weights is deferred until a forward pass actually needs them.
        model._pending = SamBaseCheckpointParams(torch.load(checkpoint_path, map_location="cpu", weights_only=True))
    return model


MASK_CC_TILE = 64                                # include/cvmi355.h CVMI_MASK_CC_TILE: the edge of the tiles the labelling runs in LDS


def get_connected_components(mask):
    """Upstream's `sam2.utils.misc.get_connected_components` (imported by sam2_infer.py:14): mask bool / u8 [N,1,H,W] on the device ->
    (labels, counts), both int32 [N,1,H,W] and 0 on background pixels; 8-connected.  A label is 1 + the flat index of the raster-first
    pixel of its component (upstream's labels are only distinct per component), counts the component's area.  Enqueued on the current
    stream (cvmi_mask_components); H and W need not be even."""
    require_gpu()
    lib = _lib.load()
    if not (torch.is_tensor(mask) and mask.is_cuda and mask.dim() == 4 and mask.shape[1] == 1 and mask.dtype in (torch.bool, torch.uint8)):
        raise TypeError("get_connected_components expects a bool / uint8 [N,1,H,W] device tensor")
    fg = mask != 0
    x = fg.float().contiguous()
    N, _, h, w = x.shape
    ws_bytes = int(lib.cvmi_mask_cc_workspace(N, h, w))
    if ws_bytes == 0:
        raise ValueError(f"get_connected_components: {N} planes of {h} x {w}: sizes must be positive and the pixel count below 2^31")
    with torch.cuda.device(x.device):
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
        labels, counts = torch.empty(N, 1, h, w, dtype=torch.int32, device=x.device), torch.empty(N, 1, h, w, dtype=torch.int32, device=x.device)
        _lib.check(lib.cvmi_mask_components(x.data_ptr(), N, h, w, 0.5, labels.data_ptr(), counts.data_ptr(), ws.data_ptr(),
                                            torch.cuda.current_stream().cuda_stream), "mask_components")
    return labels * fg, counts * fg                          # the kernel labels both phases; upstream's contract is 0 on the background


class SAM2Transforms:
    """sam2_infer.py:29-128.  `__call__` returns an f32 [3,R,R] device tensor (channels-last memory, so the model
    consumes it without a layout pass); `postprocess_masks` with the reference's settings (areas = 0) is the
    bilinear resize to the original size (:127); with max_hole_area / max_sprinkle_area > 0 every post-process first removes the small
    holes and sprinkles of the logits (:100-124, `fill_small_regions`)."""

    def __init__(self, resolution, mask_threshold, max_hole_area=0.0, max_sprinkle_area=0.0):
        self.resolution, self.mask_threshold = resolution, mask_threshold
        self.max_hole_area, self.max_sprinkle_area = max_hole_area, max_sprinkle_area
        self.mean, self.std = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]

    # Every method below behaves like a torch op: kernels are enqueued on the caller's CURRENT stream and nothing synchronises the device
    # (the first use of a result on another stream, or `.cpu()`, orders itself the usual way).  One object is shared by all session
    # threads (app.py:134): there is no shared state to protect.
    @staticmethod
    def _check_u8(x):
        img = np.ascontiguousarray(np.asarray(x))
        if img.ndim != 3 or img.shape[2] != 3 or img.dtype != np.uint8:
            raise TypeError("SAM2Transforms expects an RGB uint8 image (PIL or HxWx3 array)")
        return img

    def __call__(self, x):
        return self.forward_batch([x])[0]

    def forward_batch(self, img_list, swap_rb=False, out=None, out_dtype=F32):
        """sam2_infer.py:53-56.  -> f32 [B,3,R,R] (channels-last memory).  Equally sized images go through ONE pinned staging buffer,
        ONE H2D copy and ONE launch; so do ragged sizes, packed back to back (`detector.PackedImages`, cvmi_sam2_transform_srcs).  swap_rb: read the channels reversed (the caller's BGR2RGB,
        circuit_analyzer.py:343) instead of a host pass over every image.  out / out_dtype: write into an existing [B,R,R,3] device
        tensor of that CVMI dtype (the segmenter's input buffer) instead of a fresh f32 one."""
        require_gpu()
        lib = _lib.load()
        R = self.resolution
        imgs = [self._check_u8(im) for im in img_list]
        B = len(imgs)
        res = torch.empty(B, R, R, 3, dtype=torch.float32, device="cuda") if out is None else out
        if B and all(im.shape == imgs[0].shape for im in imgs):
            h, w = imgs[0].shape[:2]
            host = torch.empty(B, h, w, 3, dtype=torch.uint8, pin_memory=True)
            hv = host.numpy()
            for b, im in enumerate(imgs):
                hv[b] = im
            src = host.to("cuda", non_blocking=True)
            _lib.check(lib.cvmi_sam2_transform_batch(src.data_ptr(), B, h, w, res.data_ptr(), R, out_dtype, 1 if swap_rb else 0,
                                                     torch.cuda.current_stream().cuda_stream), "sam2_transform")
        elif B:                                                         # ragged: one packed upload, one launch over whole-image windows
            from .detector import PackedImages
            self._transform_srcs(PackedImages.upload(imgs, res.device), [None] * B, res, out_dtype, swap_rb)
        return res.permute(0, 3, 1, 2) if out is None else res

    def _transform_srcs(self, packed, windows, res, out_dtype, swap_rb):
        """cvmi_sam2_transform_srcs: window b (None = the whole image) of image b of a `PackedImages`, into res[b]."""
        lib = _lib.load()
        rows = np.zeros(len(packed), dtype=_lib.SAM2_SRC_ROW)
        for b, ((h, w), off, wnd) in enumerate(zip(packed.shapes, packed.offsets, windows)):
            x0, y0, x1, y1 = (0, 0, w, h) if wnd is None else wnd
            rows[b] = (off, h, w, x0, y0, x1 - x0, y1 - y0)
        _lib.check(lib.cvmi_sam2_transform_srcs(packed.data.data_ptr(), packed.data.numel(), rows.ctypes.data, len(packed), res.data_ptr(), self.resolution,
                                                out_dtype, 1 if swap_rb else 0, torch.cuda.current_stream().cuda_stream), "sam2_transform_srcs")

    def forward_windows(self, src, windows, swap_rb=False, out=None, out_dtype=F32):
        """`forward_batch` on a WINDOW of each image of a u8 [B, H, W, 3] DEVICE tensor, or of a `detector.PackedImages` (images of different
        sizes in one buffer) -- e.g. the block the detector's letterbox read, `PendingDetections.src`: windows = [(x0, y0, x1, y1) | None] per image, None = the whole image.  What the reference does with a host
        crop + a new transform (circuit_analyzer.py:1254 `image[y0:y1, x0:x1]`, then :347) is here a source rectangle of the resize kernel: no
        cropped copy, no second H2D, bit-identical to transforming a contiguous copy of the window.
        windows may also be a DEVICE int32 [B, 4] tensor of {x0, y0, w, h} rows (`glue.stage2_crop`'s `window`; u8 tensor sources only): the
        kernel reads and clips them (cvmi_sam2_transform_rects_dev), and nothing of the call depends on a value the host has seen."""
        require_gpu()
        lib = _lib.load()
        from .detector import PackedImages
        packed = isinstance(src, PackedImages)                          # images of different sizes in one packed device buffer
        if packed and not src.data.is_cuda:
            raise TypeError("forward_windows expects the PackedImages on the device")
        if not packed and not (torch.is_tensor(src) and src.is_cuda and src.dtype == torch.uint8 and src.dim() == 4 and src.shape[3] == 3 and src.is_contiguous()):
            raise TypeError("forward_windows expects a contiguous uint8 [B,H,W,3] device tensor or a PackedImages")
        B, R = len(src), self.resolution
        if len(windows) != B:
            raise ValueError("one window (or None) per image")
        res = torch.empty(B, R, R, 3, dtype=torch.float32, device=src.data.device if packed else src.device) if out is None else out
        sw, sp = 1 if swap_rb else 0, torch.cuda.current_stream().cuda_stream
        if packed:
            self._transform_srcs(src, windows, res, out_dtype, swap_rb)
        elif torch.is_tensor(windows):
            if not (windows.is_cuda and windows.dtype == torch.int32 and tuple(windows.shape) == (B, 4) and windows.is_contiguous()):
                raise TypeError("forward_windows expects device windows as a contiguous int32 [B,4] tensor of {x0, y0, w, h}")
            H, W = src.shape[1:3]
            _lib.check(lib.cvmi_sam2_transform_rects_dev(src.data_ptr(), H * W * 3, H, W, windows.data_ptr(), B, res.data_ptr(), R, out_dtype, sw, sp),
                       "sam2_transform_rects_dev")
        else:
            H, W = src.shape[1:3]
            rects = np.empty((B, 4), dtype=np.int32)
            for b, wnd in enumerate(windows):
                x0, y0, x1, y1 = (0, 0, W, H) if wnd is None else wnd
                rects[b] = (x0, y0, x1 - x0, y1 - y0)
            _lib.check(lib.cvmi_sam2_transform_rects(src.data_ptr(), H * W * 3, H, W, rects.ctypes.data, B, res.data_ptr(), R, out_dtype, sw, sp),
                       "sam2_transform_rects")
        return res.permute(0, 3, 1, 2) if out is None else res

    @property
    def fills_small_regions(self):
        return self.max_hole_area > 0 or self.max_sprinkle_area > 0

    def fill_small_regions(self, masks):
        """sam2_infer.py:100-124 on f32 [B,C,h,w] device logits, out of place: background components (8-connected, `<= mask_threshold`) of at
        most max_hole_area pixels become mask_threshold + 10, foreground components of at most max_sprinkle_area pixels mask_threshold - 10,
        both judged on the input.  Four launches on the current stream (cvmi_mask_fill_small); with both areas <= 0 the argument itself
        comes back and nothing is launched.  A failing launch raises (the reference swallows it and returns the unfiltered masks)."""
        if not self.fills_small_regions:
            return masks
        require_gpu()
        lib = _lib.load()
        if not (torch.is_tensor(masks) and masks.is_cuda and masks.dtype == torch.float32 and masks.dim() >= 2):
            raise TypeError("fill_small_regions expects an f32 [B,C,h,w] device tensor")
        m = masks.contiguous()
        h, w = m.shape[-2:]
        N = m.numel() // max(1, h * w)
        ws_bytes = int(lib.cvmi_mask_cc_workspace(N, h, w))
        if ws_bytes == 0:
            raise ValueError(f"fill_small_regions: {N} planes of {h} x {w}: sizes must be positive and the pixel count below 2^31")
        with torch.cuda.device(m.device):
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=m.device)        # torch's stream-ordered allocator owns it
            y = torch.empty_like(m)
            _lib.check(lib.cvmi_mask_fill_small(m.data_ptr(), N, h, w, float(self.mask_threshold), float(self.max_hole_area), float(self.max_sprinkle_area),
                                                y.data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream), "mask_fill_small")
        return y

    def _logits(self, masks):
        """What every post-process starts with: the logits as contiguous f32 on the device, small holes and sprinkles removed."""
        require_gpu()
        m = masks.float().contiguous()
        return self.fill_small_regions(m if m.is_cuda else m.cuda())

    def mask_return(self, logits, orig_hw=None, sizes=None, window=None, plane_stride=None, out=None):
        """The one launch under postprocess_to_mask_async / _masks_sized / _windows_async, for a caller that has run the prologue itself
        (`CircuitPipeline`): logits f32 [..., h, w], contiguous, on the device -> (u8 block, extent int32 [N,4]) on the current stream.  Exactly
        one of orig_hw = (H, W) for every plane, sizes = [(H, W)] per plane (packed back to back), window = a DEVICE int32 [N,4] tensor of
        {x0, y0, w, h} with plane n at n * plane_stride bytes.  The three resample a plane to the same bits.  out = (u8, extent): write into
        these (any shape with the bytes the form needs) instead of fresh tensors."""
        lib = _lib.load()
        h, w = logits.shape[-2:]
        N = logits.numel() // max(1, h * w)
        thr, sp = float(self.mask_threshold), torch.cuda.current_stream().cuda_stream
        u8, ext = out if out is not None else (None, torch.empty(N, 4, dtype=torch.int32, device=logits.device))
        if orig_hw is not None:
            H, W = int(orig_hw[0]), int(orig_hw[1])
            u8 = torch.empty(*logits.shape[:-2], H, W, dtype=torch.uint8, device=logits.device) if u8 is None else u8
            _lib.check(lib.cvmi_mask_postprocess(logits.data_ptr(), N, h, w, H, W, thr, u8.data_ptr(), ext.data_ptr(), sp), "mask_postprocess")
        elif sizes is not None:
            if len(sizes) != N:
                raise ValueError("one (H, W) per mask plane")
            sz = np.asarray(sizes, dtype=np.int32).reshape(N, 2)
            u8 = torch.empty(int((sz[:, 0].astype(np.int64) * sz[:, 1]).sum()), dtype=torch.uint8, device=logits.device) if u8 is None else u8
            _lib.check(lib.cvmi_mask_postprocess_sizes(logits.data_ptr(), N, h, w, sz.ctypes.data, thr, u8.data_ptr(), ext.data_ptr(), sp), "mask_postprocess_sizes")
        else:
            u8 = torch.empty(N, int(plane_stride), dtype=torch.uint8, device=logits.device) if u8 is None else u8
            _lib.check(lib.cvmi_mask_postprocess_rects_dev(logits.data_ptr(), N, h, w, window.data_ptr(), int(plane_stride), thr, u8.data_ptr(), ext.data_ptr(), sp),
                       "mask_postprocess_rects_dev")
        return u8, ext

    def postprocess_to_masks_sized(self, masks, sizes, out=None):
        """postprocess_to_mask_async for planes that return to DIFFERENT sizes (every image its own crop window): masks f32 [N,1,h,w] on the
        device, sizes = [(H, W)] per plane -> ([u8 [H_n, W_n] views of ONE packed buffer], extent int32 [N,4]); one launch, nothing copied to
        the host."""
        u8, ext = self.mask_return(self._logits(masks), sizes=sizes, out=out)
        offs = np.concatenate(([0], np.cumsum([int(H) * int(W) for H, W in sizes], dtype=np.int64)))
        return [u8.view(-1)[int(offs[n]):int(offs[n + 1])].view(int(H), int(W)) for n, (H, W) in enumerate(sizes)], ext

    def postprocess_to_windows_async(self, masks, window, plane_stride, out=None):
        """postprocess_to_mask_async with the sizes on the DEVICE: plane n returns to the {w, h} of window[n] = {x0, y0, w, h} (int32 [N,4],
        `glue.stage2_crop`'s) at the start of row n of a u8 [N, plane_stride] block (plane_stride = H0 * W0 of the uncropped image), clipped
        to its stride; no size or offset is needed on the host.  -> (the u8 block, extent int32 [N,4])."""
        return self.mask_return(self._logits(masks), window=window, plane_stride=plane_stride, out=out)

    def mask_extent(self, mask_u8):
        """Bounding boxes of binary masks [N,H,W] / [B,C,H,W] (u8 on the device): list of (x0, y0, x1, y1) or None per
        plane, with the reference's convention (circuit_analyzer.py:364-370: boundingRect of the external contours)."""
        require_gpu()
        lib = _lib.load()
        m = mask_u8.contiguous()
        H, W = m.shape[-2:]
        N = m.numel() // (H * W)
        ext = torch.empty(N, 4, dtype=torch.int32, device=m.device)
        _lib.check(lib.cvmi_mask_extent(m.data_ptr(), N, H, W, ext.data_ptr(), torch.cuda.current_stream().cuda_stream), "mask_extent")
        return self.extents_to_boxes(ext)

    @staticmethod
    def extents_to_boxes(ext):
        """int32 [N,4] {min x, min y, max x, max y} (or {W, H, -1, -1}) -> the reference's sam_extent_bbox tuples / None."""
        return [None if x1 < 0 else (x0, y0, x1 + 1, y1 + 1) for x0, y0, x1, y1 in ext.cpu().tolist()]

    # sam2_infer.py:58-86 -- what a caller needs to feed detector boxes (original pixels) to `infer_masks`
    def transform_coords(self, coords, normalize=False, orig_hw=None):
        """[..., 2] (x, y).  normalize=True: absolute pixels of an orig_hw = (h, w) image -> [0, 1] first; then x resolution."""
        coords = torch.as_tensor(coords, dtype=torch.float32)
        if normalize:
            assert orig_hw is not None
            h, w = orig_hw
            coords = coords.clone()
            coords[..., 0] = coords[..., 0] / w
            coords[..., 1] = coords[..., 1] / h
        return coords * self.resolution

    def transform_boxes(self, boxes, normalize=False, orig_hw=None):
        """[N, 4] xyxy -> [N, 2, 2] corner points in the resolution x resolution input space (as the reference returns them;
        `.reshape(-1, 4)` gives the xyxy rows `infer_masks(images, boxes)` takes)."""
        return self.transform_coords(torch.as_tensor(boxes, dtype=torch.float32).reshape(-1, 2, 2), normalize, orig_hw)

    def postprocess_masks(self, masks, orig_hw, return_u8=False):
        lib = _lib.load()
        m = self._logits(masks)
        B, C, h, w = m.shape
        H, W = int(orig_hw[0]), int(orig_hw[1])
        out = torch.empty(B, C, H, W, dtype=torch.float32, device=m.device)
        u8 = torch.empty(B, C, H, W, dtype=torch.uint8, device=m.device) if return_u8 else None
        _lib.check(lib.cvmi_bilinear_f32(m.data_ptr(), B * C, h, w, out.data_ptr(), H, W, u8.data_ptr() if return_u8 else None,
                                         float(self.mask_threshold), torch.cuda.current_stream().cuda_stream), "bilinear")
        return (out, u8) if return_u8 else out

    def postprocess_to_mask_async(self, masks, orig_hw, out=None):
        """The device half of postprocess_to_mask: -> (mask_u8 [B,C,H,W], extent int32 [B*C,4]) enqueued on the current stream, nothing
        copied to the host (extents_to_boxes(extent) does that, later, for a whole batch at once)."""
        return self.mask_return(self._logits(masks), orig_hw=orig_hw, out=out)

    def postprocess_to_mask(self, masks, orig_hw):
        """circuit_analyzer.py:354-370 in one pass on the device: bilinear resize to orig_hw -> `> mask_threshold` -> u8 {0, 255}
        -> bounding rectangle.  The f32 [B,C,H,W] map is never written; only the u8 masks and four ints per mask exist afterwards.
        Returns (mask_u8 [B,C,H,W] on the device, [(x0, y0, x1, y1) | None] per mask, the reference's `sam_extent_bbox`)."""
        u8, ext = self.postprocess_to_mask_async(masks, orig_hw)
        return u8, self.extents_to_boxes(ext)
