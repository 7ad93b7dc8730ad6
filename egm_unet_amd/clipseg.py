"""CLIPSeg (CLIPDensePredT) on the CLIP fork with the reference's constructor / forward / state_dict surface
(models/clipseg.py:136-332, 359-496), inference path on the HIP library.

    model = CLIPDensePredT(version='ViT-B/16', reduce_dim=64)       # loads weights/longclip-B.pt when present
    model.load_state_dict(torch.load('weights/rd64-uni.pth'), strict=False)
    mask_logits = model(images, prompts)[0]                          # [B, 1, H, W] fp32
"""
import os

import torch
import torch.nn as nn

from ._lib import dtype_code, lib, ptr, require_gpu, stream
from .clip import ops as O
from .clip.model import CLIP, build_model
from .clip.tokenizer import tokenize

_VIT = {"ViT-B/16": dict(patch=16, token_shape=(14, 14)), "ViT-B/32": dict(patch=32, token_shape=(7, 7))}


def get_prompt_list(prompt):
    if prompt == "plain":
        return ["{}"]
    if prompt == "fixed":
        return ["a photo of a {}."]
    if prompt == "shuffle":
        return ["a photo of a {}.", "a photograph of a {}.", "an image of a {}.", "{}."]
    if prompt == "shuffle+":
        return ["a photo of a {}.", "a photograph of a {}.", "an image of a {}.", "{}.", "a cropped photo of a {}.", "a good photo of a {}.",
                "a photo of one {}.", "a bad photo of a {}.", "a photo of the {}."]
    raise ValueError("Invalid value for prompt")


class CLIPDenseBase(nn.Module):
    """What CLIPDensePredT and CLIPDenseBaseline share (models/clipseg.py:136-332): the frozen CLIP backbone, film_mul / film_add / reduce,
    the conditionals and the encoder pass."""

    def __init__(self, version, reduce_dim, prompt, clip_weights):
        super().__init__()
        cfg = _VIT[version]
        if os.path.isfile(clip_weights):                            # models/clipseg.py:147 (hard-coded relative path there)
            self.clip_model = build_model(torch.load(clip_weights, map_location="cpu"), load_from_clip=False)
        else:                                                       # the reference ships no weights: random-init backbone of the same shape
            self.clip_model = CLIP(512, 224, 12, 768, cfg["patch"], 248, 49408, 512, 8, 12, load_from_clip=False).eval()
        self.model = self.clip_model.visual
        self.n_tokens = None
        for p in self.clip_model.parameters():
            p.requires_grad_(False)
        self.reduce_cond = None
        self.film_mul = nn.Linear(512, reduce_dim)
        self.film_add = nn.Linear(512, reduce_dim)
        self.reduce = nn.Linear(768, reduce_dim)
        self.prompt_list = get_prompt_list(prompt)
        self.precomputed_prompts = dict()
        self.compute_dtype = torch.float32

    def set_compute_dtype(self, dtype):
        self.clip_model.set_compute_dtype(dtype)
        self.compute_dtype = dtype
        return self

    # ---- conditionals (models/clipseg.py:266-332)
    @torch.no_grad()
    def compute_conditional(self, conditional):
        dev = next(self.parameters()).device
        if type(conditional) in {list, tuple}:
            # (the token tensor stays on the host: encode_text prepares ids and EOT positions there -- no cast / argmax kernels on the device)
            return self.clip_model.encode_text(tokenize(list(conditional), context_length=248, truncate=True))
        if conditional in self.precomputed_prompts:
            return self.precomputed_prompts[conditional].float().to(dev)
        return self.clip_model.encode_text(tokenize([conditional], context_length=248, truncate=True))[0]

    def get_cond_vec(self, conditional, batch_size):
        if conditional is not None and type(conditional) == str:
            return self.compute_conditional(conditional).repeat(batch_size, 1)
        if conditional is not None and type(conditional) in {list, tuple} and type(conditional[0]) == str:
            assert len(conditional) == batch_size
            return self.compute_conditional(conditional)
        if conditional is not None and type(conditional) == torch.Tensor and conditional.ndim == 2:
            return conditional
        if conditional is not None and type(conditional) == torch.Tensor:
            return self.visual_forward(conditional)[0]
        raise ValueError("invalid conditional")

    @torch.no_grad()
    def visual_forward(self, x_inp, extract_layers=(), skip=False, mask=None):
        """-> (visual_q [B, 512] fp32, activations [L, B, 768] fp32 like the reference, affinities [] (not materialised)).
        mask = (layer | 'all', 'cls_token', seg [B, H, W]): the visual-prompt mask of CLIPDensePredTMasked (models/clipseg.py:222-231):
        seg is sampled (nearest, like nnf.interpolate's default) onto the token grid and multiplies the class token's attention row
        in the selected layers."""
        q, acts = self._visual_run(x_inp, extract_layers, mask)
        return q.float(), [a.float().permute(1, 0, 2) for a in acts], []

    @torch.no_grad()
    def _visual_run(self, x_inp, extract_layers=(), mask=None, stop_after=None):
        """The encoder pass behind visual_forward in the compute dtype, batch-first: (q [B, 512], [activations [B, L, 768]]).  forward() takes
        these as they are; the reference's fp32 [L, B, 768] copies (4 x 48 MB per call at B = 32) are only made where they are returned.
        stop_after: the last block to run (q is None then)."""
        require_gpu()
        dev = self.model.conv1.weight.device
        cls_mask = None
        if mask is not None:
            mask_layer, mask_type, seg = mask
            if mask_type != "cls_token":
                raise NotImplementedError("egm_unet_amd: visual_forward masks of type 'cls_token' only (what CLIPDensePredTMasked uses)")
            g = x_inp.shape[2] // self.model.patch_size
            seg = seg.to(dev).float()
            iy = (torch.arange(g, device=dev) * seg.shape[1] // g).long()          # nearest source index = floor(dst * in / out)
            ix = (torch.arange(g, device=dev) * seg.shape[2] // g).long()
            cls_mask = (mask_layer, seg[:, iy][:, :, ix].reshape(seg.shape[0], g * g).contiguous())
        return self.model.run(x_inp.to(dev), self.compute_dtype, extract_layers=tuple(extract_layers), cls_mask=cls_mask, stop_after=stop_after)

    # ---- several prompts on one backbone pass (the reference runs the image once per prompt: predict_CLIPseg.py:495, eval_CLIPseg.py:879,
    # CLIPSegMultiLabel)
    def forward_multi(self, inp_image, conditionals):
        """inp_image [B, 3, H, W], conditionals: K prompts (a list / tuple of K strings, one string, a [K, 512] tensor, or a [K, 3, h, w]
        image tensor that goes through visual_forward) -> fp32 logits [B, K, H', W'] with out[b, k] = self(inp_image[b:b+1], prompt k)[0][0, 0].
        The backbone runs once per image (plus once per image conditional) and stops after the last layer the decoder reads; only the
        decoder runs per (image, prompt).  Inference only."""
        if self.training and torch.is_grad_enabled():
            raise NotImplementedError("egm_unet_amd: forward_multi is inference only (call .eval() or run under torch.no_grad())")
        with torch.no_grad():
            dev = self.model.positional_embedding.device
            x_inp = inp_image.to(dev)
            if x_inp.ndim != 4:
                raise ValueError(f"forward_multi: inp_image must be [B, 3, H, W], got {tuple(x_inp.shape)}")
            cond = self._multi_cond(conditionals)
            condT = self._cond_in_dtype(cond)
            out = self._decode_multi(x_inp, condT)
            B, K = x_inp.shape[0], cond.shape[0]
            return out.view(B, K, out.shape[-2], out.shape[-1])

    def forward_multi_train(self, inp_image, conditionals):
        """forward_multi for decoder training: the same inputs -> fp32 logits [B, K, H', W'] with out[b, k] = self(inp_image[b:b+1],
        prompt k)[0][0, 0] in train mode, differentiable in the decoder parameters (their gradients equal those of the repeat form, the
        image fed once per prompt); the conditionals are constants.  The frozen backbone runs once per image under no_grad and stops
        after the last layer the decoder reads; the decoder's dropout draws its masks for the B*K sequences.  In eval mode or with
        autograd off this is forward_multi.  Loss: clip.train_ops.bce_with_logits(out, target [B, K, H', W']), to which
        train_utils.LovaszHinge().loss(out, target) adds the IoU surrogate of every (b, k) map."""
        if not (self.training and torch.is_grad_enabled()):
            return self.forward_multi(inp_image, conditionals)
        dev = self.model.positional_embedding.device
        x_inp = inp_image.to(dev)
        if x_inp.ndim != 4:
            raise ValueError(f"forward_multi_train: inp_image must be [B, 3, H, W], got {tuple(x_inp.shape)}")
        with torch.no_grad():
            cond = self._multi_cond(conditionals)
            condT = self._cond_in_dtype(cond)
        from .clip.train_ops import DECODER as T
        out = self._decode_multi(x_inp, condT, T)
        B, K = x_inp.shape[0], cond.shape[0]
        return out.view(B, K, out.shape[-2], out.shape[-1])

    def _multi_cond(self, conditionals):
        """The K conditional vectors [K, 512] fp32 of forward_multi (get_cond_vec's forms, K in place of the batch size)."""
        width = self.film_mul.in_features
        if isinstance(conditionals, str):
            return self.compute_conditional(conditionals).reshape(1, -1)
        if isinstance(conditionals, (list, tuple)):
            if len(conditionals) == 0:
                raise ValueError("forward_multi: no conditionals given")
            if not all(isinstance(c, str) for c in conditionals):
                raise ValueError("forward_multi: a list of conditionals must hold strings only")
            return self.compute_conditional(list(conditionals))
        if isinstance(conditionals, torch.Tensor):
            if conditionals.shape[0] == 0:
                raise ValueError("forward_multi: no conditionals given")
            if conditionals.ndim == 2:
                if conditionals.shape[1] != width:
                    raise ValueError(f"forward_multi: conditional vectors must be [K, {width}], got {tuple(conditionals.shape)}")
                return conditionals.to(self.model.positional_embedding.device).float()
            if conditionals.ndim == 4:
                return self.visual_forward(conditionals)[0]
            raise ValueError(f"forward_multi: a conditional tensor must be [K, {width}] or [K, 3, h, w], got {tuple(conditionals.shape)}")
        raise ValueError("forward_multi: invalid conditionals")

    def _cond_in_dtype(self, cond):
        """The conditional vectors [B, 512] fp32 -> the compute dtype (the film linears' input)."""
        condT = torch.empty(cond.shape, dtype=self.compute_dtype, device=cond.device)
        lib().call("egm_cast_f32", dtype_code(self.compute_dtype), ptr(cond.float().contiguous()), ptr(condT), cond.numel(), stream())
        return condT

    def _film_vecs(self, ops, condT):
        """(mul, add) = (film_mul, film_add) of the conditional vectors [N, 512] -> [N, rd] each."""
        return ops.linear(condT, self.film_mul.weight, self.film_mul.bias), ops.linear(condT, self.film_add.weight, self.film_add.bias)

    def _features(self, out, q_raw, cond, acts, return_features):
        """forward()'s result: (logits,) or, with return_features, the reference's (logits, visual_q, cond, fp32 [L, B, 768] activations)."""
        if return_features:
            return out, q_raw.float(), cond, [t.float().permute(1, 0, 2) for t in acts]
        return out,


class CLIPDensePredT(CLIPDenseBase):
    def __init__(self, version="ViT-B/32", extract_layers=(3, 6, 9), cond_layer=0, reduce_dim=128, n_heads=4, prompt="fixed", extra_blocks=0,
                 reduce_cond=None, fix_shift=False, learn_trans_conv_only=False, limit_to_clip_only=False, upsample=False,
                 add_calibration=False, rev_activations=False, trans_conv=None, n_tokens=None, complex_trans_conv=False,
                 clip_weights="weights/longclip-B.pt"):
        for flag, name in ((extra_blocks, "extra_blocks"), (reduce_cond, "reduce_cond"), (fix_shift, "fix_shift"), (upsample, "upsample"),
                           (n_tokens, "n_tokens"), (trans_conv, "trans_conv")):
            if flag:
                raise NotImplementedError(f"egm_unet_amd: CLIPDensePredT({name}=...) is not used by the reference scripts and not implemented")
        super().__init__(version, reduce_dim, prompt, clip_weights)
        cfg = _VIT[version]
        self.extract_layers, self.cond_layer = extract_layers, cond_layer
        self.limit_to_clip_only, self.process_cond, self.rev_activations = limit_to_clip_only, None, rev_activations
        self.upsample_proj, self.add_activation1, self.version = None, True, version
        self.token_shape = cfg["token_shape"]
        self.shift_vector = None
        ks = (cfg["patch"], cfg["patch"])
        self.complex_trans_conv = bool(complex_trans_conv)
        if not complex_trans_conv:
            self.trans_conv = nn.ConvTranspose2d(reduce_dim, 1, ks, stride=ks)
        else:                                                       # models/clipseg.py:403-414, the rd64-uni-refined checkpoint
            if cfg["patch"] != 16 or reduce_dim not in (64, 128):
                raise NotImplementedError(f"egm_unet_amd: complex_trans_conv needs ViT-B/16 and reduce_dim 64 or 128 (got {version}, {reduce_dim})")
            tp = cfg["patch"] // 4
            self.trans_conv = nn.Sequential(
                nn.Conv2d(reduce_dim, reduce_dim, kernel_size=3, padding=1),
                nn.ReLU(),
                nn.ConvTranspose2d(reduce_dim, reduce_dim // 2, kernel_size=tp, stride=tp),
                nn.ReLU(),
                nn.ConvTranspose2d(reduce_dim // 2, 1, kernel_size=tp, stride=tp),
            )
        depth = len(extract_layers)
        self.reduces = nn.ModuleList([nn.Linear(768, reduce_dim) for _ in range(depth)])
        self.blocks = nn.ModuleList([nn.TransformerEncoderLayer(d_model=reduce_dim, nhead=n_heads) for _ in range(depth)])
        self.extra_blocks = nn.ModuleList([])
        self.n_heads = n_heads
        self.decoder_dropout = None          # None: the encoder layers' own p (0.1, as in the reference's train mode); 0.0 disables it

    def _encoder_layer(self, ops, blk, a, p):
        """nn.TransformerEncoderLayer defaults (post-norm, ReLU feed-forward) with dropout p on the attention weights, behind the attention
        output projection, behind the ReLU and behind the second feed-forward linear (models/clipseg.py:421-422); p = 0: eval mode."""
        at = blk.self_attn
        att = ops.self_attention(ops.linear(a, at.in_proj_weight, at.in_proj_bias), self.n_heads, p)
        a = ops.layernorm(ops.linear_dropout(att, at.out_proj.weight, at.out_proj.bias, p, 0, a), blk.norm1)
        h = ops.linear_dropout(a, blk.linear1.weight, blk.linear1.bias, p, 1)
        return ops.layernorm(ops.linear_dropout(h, blk.linear2.weight, blk.linear2.bias, p, 0, a), blk.norm2)

    def forward(self, inp_image, conditional=None, return_features=False, mask=None):
        """models/clipseg.py:436-496.  eval(): inference path, no autograd.  train(): the decoder (reduces, FiLM, blocks, trans_conv)
        is differentiable through the HIP autograd operators of clip/train_ops.py; the CLIP backbone stays frozen (:155-156);
        nn.TransformerEncoderLayer's dropout is applied (self.decoder_dropout overrides its p; 0.0 switches it off)."""
        assert type(return_features) == bool
        if mask is not None:
            raise ValueError("mask not supported")                  # as the reference (models/clipseg.py:442-443)
        train = self.training and torch.is_grad_enabled()
        with torch.no_grad():
            x_inp = inp_image.to(self.model.positional_embedding.device)
            cond = self.get_cond_vec(conditional, x_inp.shape[0])
            q_raw, acts_all = self._visual_run(x_inp, extract_layers=[0] + list(self.extract_layers))
            condT = self._cond_in_dtype(cond)
            if not train:
                out = self._decode(O.DECODER, acts_all[1:], condT, False)
        if train:
            from .clip.train_ops import DECODER as T
            out = self._decode(T, [t.detach() for t in acts_all[1:]], condT, False)
        return self._features(out, q_raw, cond, acts_all, return_features)

    def _decode(self, ops, acts, condT, fan):
        """The decoder on the operator set ops (clip/ops.DECODER or clip/train_ops.DECODER): per extracted layer reduce_i(act_i) + the
        running a, FiLM at cond_layer, an encoder layer; then trans_conv or the refined head -> fp32 [N, 1, H', W'].
        fan = False: condT [B, 512], one conditional per image, N = B.
        fan = True: condT [K, 512], every image with every prompt, N = B*K.  The layers before cond_layer run on the B sequences; at
        cond_layer one fan-out kernel writes a[b*K + k] = mul[k] * r[b] + add[k]; behind it reduce_i(act_i) stays a product over B*L
        rows whose result is broadcast-added into the B*K sequences (so are its gradients: summed over the prompts)."""
        acts = acts if self.rev_activations else acts[::-1]
        a, fanned = None, False
        for i, (act, blk, red) in enumerate(zip(acts, self.blocks, self.reduces)):
            if fanned:
                a = ops.add_fan(a, ops.linear(act, red.weight, red.bias))
            else:
                a = ops.linear(act, red.weight, red.bias, residual=a)
                if i == self.cond_layer:
                    a = (ops.film_fan if fan else ops.film)(a, *self._film_vecs(ops, condT))
                    fanned = fan
            p = 0.0 if not ops.training else self.decoder_dropout if self.decoder_dropout is not None else float(blk.dropout.p)
            a = self._encoder_layer(ops, blk, a, p)
        if fan and not fanned:                                       # cond_layer behind the last layer: no FiLM, every prompt alike
            one = torch.ones((condT.shape[0], a.shape[-1]), dtype=a.dtype, device=a.device)
            a = ops.film_fan(a, one, torch.zeros_like(one))
        if self.complex_trans_conv:
            return ops.refine(a, self.trans_conv)
        return ops.trans_conv(a, self.trans_conv.weight, self.trans_conv.bias)

    def _decode_multi(self, x_inp, condT, ops=O.DECODER):
        """forward_multi's (ops = clip/train_ops.DECODER: forward_multi_train's) backbone pass and decoder -> fp32 [B*K, 1, H', W']."""
        _, acts_all = self._visual_run(x_inp, extract_layers=[0] + list(self.extract_layers), stop_after=max(self.extract_layers))
        return self._decode(ops, [t.detach() for t in acts_all[1:]] if ops.training else acts_all[1:], condT, True)


class CLIPDensePredTMasked(CLIPDensePredT):
    """CLIPSeg conditioned on a support image + its segmentation (models/clipseg.py:500-525): the conditional vector is the CLIP
    image feature of the support image, computed with the class token's attention restricted to the masked region in every layer."""

    def __init__(self, version="ViT-B/32", extract_layers=(3, 6, 9), cond_layer=0, reduce_dim=128, n_heads=4, prompt="fixed", extra_blocks=0,
                 reduce_cond=None, fix_shift=False, learn_trans_conv_only=False, refine=None, limit_to_clip_only=False, upsample=False,
                 add_calibration=False, n_tokens=None, **kw):
        super().__init__(version=version, extract_layers=extract_layers, cond_layer=cond_layer, reduce_dim=reduce_dim, n_heads=n_heads,
                         prompt=prompt, extra_blocks=extra_blocks, reduce_cond=reduce_cond, fix_shift=fix_shift,
                         learn_trans_conv_only=learn_trans_conv_only, limit_to_clip_only=limit_to_clip_only, upsample=upsample,
                         add_calibration=add_calibration, n_tokens=n_tokens, **kw)

    def visual_forward_masked(self, img_s, seg_s):
        return super().visual_forward(img_s, mask=("all", "cls_token", seg_s))

    def forward(self, img_q, cond_or_img_s, seg_s=None, return_features=False):
        if seg_s is None:
            cond = cond_or_img_s
        else:
            with torch.no_grad():
                cond, _, _ = self.visual_forward_masked(cond_or_img_s, seg_s)
        return super().forward(img_q, cond, return_features=return_features)


BASELINE_FUSED = os.environ.get("EGM_CLIPSEG_BL_FUSED", "1") != "0"     # False: the head runs on the composed operators (A/B, cross-check)


class CLIPDenseBaseline(CLIPDenseBase):
    """CLIPSeg's baseline (models/clipseg.py:529-590; experiments/phrasecut.yaml:81, coco.yaml:98-101, pascal_1shot.yaml:92-95): the layer
    extract_layer activation -> reduce -> FiLM -> reduce2 (Linear, ReLU, Linear) -> ConvTranspose2d per token, no transformer decoder.
    bf16 with patch 16 and reduce dims that are multiples of 16 up to 128: one fused HIP launch (csrc/clipseg_baseline.hip, training:
    clip/train_ops.BaselineHeadFn); fp32, other shapes or BASELINE_FUSED = False: the composed operators.  Without return_features the
    backbone stops after extract_layer (visual_q is not computed)."""

    def __init__(self, version="ViT-B/32", cond_layer=0, extract_layer=9, reduce_dim=128, reduce2_dim=None, prompt="fixed", reduce_cond=None,
                 limit_to_clip_only=False, n_tokens=None, clip_weights="weights/longclip-B.pt"):
        for flag, name in ((reduce_cond, "reduce_cond"), (n_tokens, "n_tokens")):
            if flag:
                raise NotImplementedError(f"egm_unet_amd: CLIPDenseBaseline({name}=...) is not used by the reference scripts and not implemented")
        super().__init__(version, reduce_dim, prompt, clip_weights)
        self.extract_layer = extract_layer
        self.limit_to_clip_only = limit_to_clip_only
        self.shift_vector = None
        self.token_shape = _VIT[version]["token_shape"]
        assert reduce2_dim is not None                              # as the reference (models/clipseg.py:546)
        self.reduce2 = nn.Sequential(nn.Linear(reduce_dim, reduce2_dim), nn.ReLU(), nn.Linear(reduce2_dim, reduce_dim))
        ks = (_VIT[version]["patch"], _VIT[version]["patch"])
        self.trans_conv = nn.ConvTranspose2d(reduce_dim, 1, ks, stride=ks)

    def _fused(self):
        return BASELINE_FUSED and O.baseline_supported(self.reduce.weight.shape[0], self.reduce2[0].weight.shape[0], self.trans_conv.kernel_size[0],
                                                       self.compute_dtype)

    def forward(self, inp_image, conditional=None, return_features=False):
        """models/clipseg.py:556-590.  eval(): inference, no autograd.  train(): film_mul / film_add / reduce / reduce2 / trans_conv are
        differentiable through the HIP operators of clip/train_ops.py; the CLIP backbone stays frozen."""
        assert type(return_features) == bool
        x_inp = inp_image.to(self.model.positional_embedding.device)
        train = self.training and torch.is_grad_enabled()
        with torch.no_grad():
            cond = self.get_cond_vec(conditional, x_inp.shape[0])
            q_raw, acts = self._visual_run(x_inp, [self.extract_layer], stop_after=None if return_features else self.extract_layer)
            condT = self._cond_in_dtype(cond)
            if not train:
                out = self._head(O.DECODER, acts[0], *self._film_vecs(O.DECODER, condT), False)
        if train:
            from .clip.train_ops import DECODER as T
            out = self._head(T, acts[0].detach(), *self._film_vecs(T, condT), False)
        return self._features(out, q_raw, cond, acts, return_features)

    def _head(self, ops, act, mul, add, fan):
        """reduce -> FiLM -> reduce2 -> trans_conv on the operator set ops: the fused launch where it exists, else composed.
        fan = False: mul / add [B, rd], one conditional per image -> fp32 [B, 1, H', W'].
        fan = True: mul / add [K, rd], every image with every prompt; fused (inference only: reduce once per token tile) -> [B, K, H', W'],
        composed (reduce on B*L rows, the FiLM fan-out, reduce2 / trans_conv on B*K sequences) -> [B*K, 1, H', W']."""
        if self._fused() and not (fan and ops.training):
            return ops.baseline_fused(act, mul, add, self.reduce, self.reduce2, self.trans_conv, fan)
        a = (ops.film_fan if fan else ops.film)(ops.linear(act, self.reduce.weight, self.reduce.bias), mul, add)
        a = ops.linear(a, self.reduce2[0].weight, self.reduce2[0].bias, act=1)
        a = ops.linear(a, self.reduce2[2].weight, self.reduce2[2].bias)
        return ops.trans_conv(a, self.trans_conv.weight, self.trans_conv.bias)

    def _decode_multi(self, x_inp, condT, ops=O.DECODER):
        """forward_multi's (ops = clip/train_ops.DECODER: forward_multi_train's) head: the backbone once, stopping after extract_layer."""
        _, acts = self._visual_run(x_inp, [self.extract_layer], stop_after=self.extract_layer)
        return self._head(ops, acts[0].detach() if ops.training else acts[0], *self._film_vecs(ops, condT), True)


# 'background' + datasets/pascal_classes.json in id order (the reference's third_party.JoEm VOC list, which its tree does not ship)
PASCAL_CLASSES = ("background", "aeroplane", "bicycle", "bird", "boat", "bottle", "bus", "car", "cat", "chair", "cow", "diningtable", "dog",
                  "horse", "motorbike", "person", "pottedplant", "sheep", "sofa", "train", "tvmonitor")


class CLIPSegMultiLabel(nn.Module):
    """models/clipseg.py:592-625: the 21 PASCAL classes as bare-name prompts on one image batch -> [B, 21, 352, 352] with
    out[:, c] = -10 + fac_c * sigmoid(logits_c), fac = 3 for background, 1 otherwise.  One forward_multi call (the backbone runs once
    per image, not once per class), then one in-place sigmoid / scale / offset kernel.
    model: a CLIPDenseBase instance, or the path of a decoder state dict loaded with strict=False into
    CLIPDensePredT(version='ViT-B/16', reduce_dim=64) (what the reference's load_model does for its checkpoints, predict_CLIPseg.py:413-415)."""

    SIZE = 352                                                      # the reference's output buffer (models/clipseg.py:611)

    def __init__(self, model):
        super().__init__()
        self.pascal_classes = PASCAL_CLASSES
        if isinstance(model, CLIPDenseBase):
            self.clipseg = model
        elif isinstance(model, (str, os.PathLike)):
            self.clipseg = CLIPDensePredT(version="ViT-B/16", reduce_dim=64)
            self.clipseg.load_state_dict(torch.load(model, map_location="cpu"), strict=False)
        else:
            raise TypeError(f"CLIPSegMultiLabel: model must be a CLIPDenseBase or a state-dict path, got {type(model).__name__}")
        self.clipseg.eval()
        self._fac = {}

    def forward(self, x):
        P = self.clipseg.model.patch_size
        H, W = x.shape[-2] // P * P, x.shape[-1] // P * P
        if (H, W) != (self.SIZE, self.SIZE):
            raise ValueError(f"CLIPSegMultiLabel: the logits are {H} x {W}; the reference's output is fixed at {self.SIZE} x {self.SIZE} "
                             f"(input {x.shape[-2]} x {x.shape[-1]})")
        out = self.clipseg.forward_multi(x, list(self.pascal_classes))                   # [B, 21, 352, 352] fp32
        fac = self._fac.get(out.device)
        if fac is None:
            fac = torch.tensor([3.0 if c == "background" else 1.0 for c in self.pascal_classes], device=out.device)
            self._fac[out.device] = fac
        return O.sigmoid_affine_(out, fac, -10.0)
