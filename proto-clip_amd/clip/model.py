"""CLIP towers on the gfx950 kernels (reference clip/model.py:155-434).

`build_model(state_dict)` accepts an OpenAI-format CLIP state dict (same key names the reference's
`build_model` consumes, clip/model.py:397-434) and returns an object with the reference's surface:
`encode_image`, `encode_text`, `dtype`, `eval()`, `state_dict()`, `visual.input_resolution`.
Parameters live in an nn.Module tree with the reference's names, so `load_state_dict` of real OpenAI
weights works unchanged; the forward passes are sequences of libpclip launches (MFMA linears with
fused bias/QuickGELU/residual epilogues, fp32-statistics LayerNorm, whole-sequence attention).

Precision follows `convert_weights` (clip/model.py:373-394): Linear/conv/projection weights fp16,
LayerNorm and embedding parameters fp32, activations fp16 with fp32 accumulation.
Both vision towers are built: VisionTransformer (ViT-B/32, ViT-B/16, ViT-L/14) and ModifiedResNet (RN50 / RN101 /
RN50x4 / RN50x16: NHWC activations, 1x1 convs as GEMMs and 3x3 convs as implicit GEMMs with the eval BatchNorm (+ReLU) in
their epilogue; im2col + GEMM only for the strided 3-channel first convolution of the stem)."""
import os
from collections import OrderedDict

import numpy as np
import torch
from torch import nn

from .. import ops
from .._lib import PclipError
from ..tower import Tower, _run_blocks, class_row_pick, eot_row_pick, run_tower, vit_stem  # noqa: F401  (_run_blocks: tools/tower_backward_bench.py imports it here)


class _Box(nn.Module):
    """Parameter container; attribute names mirror the reference's module tree."""


def _linear(out_f, in_f, bias=True):
    b = _Box()
    b.weight = nn.Parameter(torch.empty(out_f, in_f), requires_grad=False)
    if bias:
        b.bias = nn.Parameter(torch.empty(out_f), requires_grad=False)
    return b


def _ln(width):
    b = _Box()
    b.weight = nn.Parameter(torch.ones(width), requires_grad=False)
    b.bias = nn.Parameter(torch.zeros(width), requires_grad=False)
    return b


def _resblock(width):
    blk = _Box()
    blk.attn = _Box()
    blk.attn.in_proj_weight = nn.Parameter(torch.empty(3 * width, width), requires_grad=False)
    blk.attn.in_proj_bias = nn.Parameter(torch.zeros(3 * width), requires_grad=False)
    blk.attn.out_proj = _linear(width, width)
    blk.ln_1 = _ln(width)
    blk.mlp = _Box()
    blk.mlp.c_fc = _linear(4 * width, width)
    blk.mlp.c_proj = _linear(width, 4 * width)
    blk.ln_2 = _ln(width)
    return blk


def _transformer(width, layers):
    t = _Box()
    t.width, t.layers = width, layers
    t.resblocks = nn.Sequential(*[_resblock(width) for _ in range(layers)])
    return t


# (Rounds 2 - 5 carried two opt-in forms of the LayerNorms — folded into the consuming linear (PCLIP_LN_FOLD=1: an independent rounding, +3.5 % in round 3, -0.9 % against
# the four-wave GEMM of round 5) and computed inside the residual GEMM's launch (PCLIP_RES_LN_FUSE=1: same bits, -1.2 %).  Both lost to the plain LayerNorm pass and
# were removed in round 6: profiles/r03_e2e_fold_study.json, r04_ab_res_ln.txt, r06_bench_v0.json.)


class _Cached:
    """Derived (cast / transposed / padded) copies of parameters, refreshed when the source changes."""

    def __init__(self):
        self._c = {}

    def get(self, key, src, fn):
        tag = (src.data_ptr(), src._version, src.dtype, src.device)
        hit = self._c.get(key)
        if hit is None or hit[0] != tag:
            hit = (tag, fn(src.detach()))
            self._c[key] = hit
        return hit[1]


class VisionTransformer(nn.Module):
    """clip/model.py:204-238."""

    def __init__(self, input_resolution, patch_size, width, layers, heads, output_dim):
        super().__init__()
        self.input_resolution, self.patch_size = input_resolution, patch_size
        self.width, self.heads, self.output_dim = width, heads, output_dim
        self.conv1 = _Box()
        self.conv1.weight = nn.Parameter(torch.empty(width, 3, patch_size, patch_size), requires_grad=False)
        self.class_embedding = nn.Parameter(torch.empty(width), requires_grad=False)
        self.positional_embedding = nn.Parameter(torch.empty((input_resolution // patch_size) ** 2 + 1, width),
                                                 requires_grad=False)
        self.ln_pre = _ln(width)
        self.transformer = _transformer(width, layers)
        self.ln_post = _ln(width)
        self.proj = nn.Parameter(torch.empty(width, output_dim), requires_grad=False)
        self._cache = _Cached()
        prefix = [("visual.conv1.weight", self.conv1.weight), ("visual.class_embedding", self.class_embedding),           # VitStemFn's argument order
                  ("visual.positional_embedding", self.positional_embedding), ("visual.ln_pre.weight", self.ln_pre.weight),
                  ("visual.ln_pre.bias", self.ln_pre.bias)]
        head = [("visual.ln_post.weight", self.ln_post.weight), ("visual.ln_post.bias", self.ln_post.bias), ("visual.proj", self.proj)]
        self.tower = Tower("encode_image", "visual tower", "stem", blocks=self.transformer.resblocks, heads=heads, causal=False, ln=self.ln_post,
                           proj=self.proj, cache=self._cache, projT_key="projT", prefix=prefix, head=head, pick=class_row_pick)
        # images per pass: bounds activation memory (c_fc output = chunk*L*4W*2 B = 1.2 GB for ViT-B/16 at 1024);
        # larger passes waste less of the GEMMs' last round of persistent tiles (measured on MI355X: 1024 > 512 > 256)
        self.chunk = int(os.environ.get("PCLIP_VIT_CHUNK", "1024"))

    def forward(self, x: torch.Tensor):
        if x.dim() != 4 or x.shape[1] != 3 or x.shape[2] != self.input_resolution or x.shape[3] != self.input_resolution:
            raise PclipError(f"expected images [B,3,{self.input_resolution},{self.input_resolution}], got {tuple(x.shape)}")
        outs = [self._forward_chunk(x[i:i + self.chunk]) for i in range(0, x.shape[0], self.chunk)]
        return outs[0] if len(outs) == 1 else torch.cat(outs, dim=0)

    @property
    def _stem_opt_in(self):
        """CLIP.unfreeze(stem=...) has opted the prefix in: conv1 / embeddings / ln_pre may train."""
        return self.tower.stem_opt_in

    @_stem_opt_in.setter
    def _stem_opt_in(self, value):
        self.tower.stem_opt_in = bool(value)

    def _tape_from(self):
        """Index of the first residual block with a trainable parameter (layers: only ln_post / proj train), None when the tower is frozen.
        Refuses a trainable prefix parameter, opted in or not: the taped passes plan with `_tape_plan`."""
        return self.tower.tape_from()

    def _tape_plan(self):
        """(first, stem): `_tape_from`, except that prefix parameters opted in through CLIP.unfreeze(stem=...) put the whole tower on the tape."""
        return self.tower.tape_plan()

    def _forward_chunk(self, img):
        P, tw = self.patch_size, self.tower
        G = self.input_resolution // P
        if img.dtype not in (torch.float32, torch.float16):   # fp32: image.type(self.dtype) (clip/model.py:339) rides on the im2col gather
            raise PclipError(f"unsupported image dtype {img.dtype}")
        img = img.contiguous()
        plan = tw.tape_plan() if torch.is_grad_enabled() else (None, False)
        stem_in = (img, self.conv1.weight, self.class_embedding, self.positional_embedding)
        h0 = None
        if plan[1]:                                                         # whole-tower fine-tuning: the stem and every block on the tape
            from ..autograd import VitStemFn
            x = VitStemFn.apply(*stem_in, self.ln_pre.weight, self.ln_pre.bias, P, self._cache)
        elif len(tw.blocks) > 0:                                            # tokens + ln_pre + the first block's ln_1 in one pass
            ln_1 = tw.blocks[0].ln_1
            x, h0 = vit_stem(self._cache, *stem_in, P, fused=(self.ln_pre.weight, self.ln_pre.bias, ln_1.weight, ln_1.bias))
        else:
            x = ops.layernorm(vit_stem(self._cache, *stem_in, P), self.ln_pre.weight, self.ln_pre.bias)      # clip/model.py:227
        B, L = img.shape[0], G * G + 1
        return run_tower(tw, x, B, L, plan, tw.pick(B, L, x.device), h0=h0)                  # 229-236


def _bn(ch):
    b = _Box()
    b.weight = nn.Parameter(torch.ones(ch), requires_grad=False)
    b.bias = nn.Parameter(torch.zeros(ch), requires_grad=False)
    b.register_buffer("running_mean", torch.zeros(ch))
    b.register_buffer("running_var", torch.ones(ch))
    b.register_buffer("num_batches_tracked", torch.tensor(0, dtype=torch.long))
    b.eps = 1e-5
    return b


def _conv(cout, cin, k):
    b = _Box()
    b.weight = nn.Parameter(torch.empty(cout, cin, k, k), requires_grad=False)
    return b


class _Bottleneck(_Box):
    """Parameter tree of clip/model.py:10-38 (conv1 1x1, conv2 3x3, avgpool(stride), conv3 1x1, optional
    downsample = avgpool(stride) -> 1x1 conv -> bn, whose Sequential keys are '0' and '1')."""

    def __init__(self, inplanes, planes, stride):
        super().__init__()
        self.conv1, self.bn1 = _conv(planes, inplanes, 1), _bn(planes)
        self.conv2, self.bn2 = _conv(planes, planes, 3), _bn(planes)
        self.conv3, self.bn3 = _conv(planes * 4, planes, 1), _bn(planes * 4)
        self.stride = stride
        self.downsample = None
        if stride > 1 or inplanes != planes * 4:
            self.downsample = nn.ModuleDict({"0": _conv(planes * 4, inplanes, 1), "1": _bn(planes * 4)})


class ModifiedResNet(nn.Module):
    """clip/model.py:95-152 on the gfx950 kernels.  Activations are NHWC fp16 rows [B*H*W, C]: 1x1 convolutions are
    plain MFMA GEMMs (K a multiple of 8: the 80 / 96 / 160-channel inputs of RN50x4 / x16 take the GEMM's K-tail
    instantiations), stride-1 3x3 convolutions are implicit GEMMs for any channel counts that are multiples of 8, and only
    the stride-2 3-channel stem convolution goes through an im2col matrix.  BatchNorm(eval) + ReLU (+ residual) rides in
    the GEMM epilogues; the attention pool reuses the transformer attention kernel (head dim 64)."""

    def __init__(self, layers, output_dim, heads, input_resolution=224, width=64):
        super().__init__()
        self.output_dim, self.input_resolution, self.heads = output_dim, input_resolution, heads
        self.conv1, self.bn1 = _conv(width // 2, 3, 3), _bn(width // 2)
        self.conv2, self.bn2 = _conv(width // 2, width // 2, 3), _bn(width // 2)
        self.conv3, self.bn3 = _conv(width, width // 2, 3), _bn(width)
        inpl = width
        for li, (planes, nblk, stride) in enumerate(zip((width, width * 2, width * 4, width * 8), layers, (1, 2, 2, 2)), 1):
            blocks = [_Bottleneck(inpl, planes, stride)]
            inpl = planes * 4
            blocks += [_Bottleneck(inpl, planes, 1) for _ in range(1, nblk)]
            setattr(self, f"layer{li}", nn.Sequential(*blocks))
        embed = width * 32
        if embed // heads != 64:
            raise PclipError(f"attention pool head dim {embed // heads} unsupported (the attention kernel needs 64)")
        self.attnpool = _Box()
        self.attnpool.positional_embedding = nn.Parameter(torch.empty((input_resolution // 32) ** 2 + 1, embed), requires_grad=False)
        for nm in ("k_proj", "q_proj", "v_proj"):
            setattr(self.attnpool, nm, _linear(embed, embed))
        self.attnpool.c_proj = _linear(output_dim, embed)
        self._cache = _Cached()
        # images per pass: small passes are launch-bound and leave the tail tiles of every convolution idle — 1024 images in passes of 128 / 256 / 512 / 1024:
        # RN50 33.4 / 37.0 / 39.6 / 41.6 k img/s, RN101 22.5 / 25.7 / 27.0 / 28.5 k (profiles/r06_rn_chunk_probe.txt); the widest activation of a 1024-image pass
        # (layer1's 56 x 56 x 256 fp16) is 1.6 GB.  Same bits for every pass size (tests/test_gpu_encoder.py).
        # (RN50x4 / x16 — 40 / 48 stem channels — keep passes of 256: their stem convolution still goes through an im2col matrix (288 / 384 px, no fused stem
        # kernel), 4 - 9 GB for a 1024-image pass, and their widest activation at 1024 images is 4 - 7 GB.  Same bits for every pass size.)
        self.chunk = int(os.environ.get("PCLIP_RN_CHUNK", "1024" if width // 2 in (32, 64) else "256"))

    # -- helpers ---------------------------------------------------------------------------------------------------
    def _bn_affine(self, key, bn):
        def fold(_):
            inv = torch.rsqrt(bn.running_var.float() + bn.eps)
            scale = bn.weight.float() * inv
            return torch.stack([scale, bn.bias.float() - bn.running_mean.float() * scale]).contiguous()
        tag_src = bn.weight            # refreshed when the affine weight tensor is replaced; running stats are frozen in eval
        ss = self._cache.get(("bn", key), tag_src, fold)
        return ss[0], ss[1]

    def _w1x1(self, key, conv):
        return self._cache.get(("w1", key), conv.weight, lambda w: w.reshape(w.shape[0], w.shape[1]).contiguous())

    def _w3x3(self, key, conv):
        def prep(w):                   # [Cout, Cin, 3, 3] -> [Cout, (ky, kx, Cin)] padded to the GEMM's K-tile
            co, ci = w.shape[0], w.shape[1]
            w2 = w.permute(0, 2, 3, 1).reshape(co, 9 * ci)
            kpad = (9 * ci + 63) // 64 * 64
            if kpad != 9 * ci:
                w2 = torch.cat([w2, w2.new_zeros(co, kpad - 9 * ci)], dim=1)
            return w2.contiguous()
        return self._cache.get(("w3", key), conv.weight, prep)

    def _conv3_bn_relu(self, key, x, strides, B, H, W, C, conv, bn, stride=1):
        sc, sh = self._bn_affine(key, bn)
        if stride == 1 and C % 8 == 0 and conv.weight.shape[0] % 8 == 0 and strides == (H * W * C, W * C, C, 1):
            return ops.conv3x3_bn(x, self._w3x3(key, conv), sc, sh, B, H, W, C, relu=True)   # implicit GEMM: no im2col buffer
        cols = ops.im2col3x3(x, strides, B, H, W, C, stride)
        return ops.gemm_bn(cols, self._w3x3(key, conv), sc, sh, relu=True)                   # relu(bn(conv3x3(x))) in one launch

    def _bottleneck(self, key, blk, x, B, H, W, Cin):
        planes = blk.conv1.weight.shape[0]
        sc, sh = self._bn_affine(key + ".1", blk.bn1)
        out = ops.gemm_bn(x, self._w1x1(key + ".1", blk.conv1), sc, sh, relu=True)           # relu(bn1(conv1(x)))
        out = self._conv3_bn_relu(key + ".2", out, (H * W * planes, W * planes, planes, 1), B, H, W, planes, blk.conv2, blk.bn2)
        Ho, Wo = H, W
        if blk.stride > 1:
            out = ops.avgpool_nhwc(out, B, H, W, planes, blk.stride)                         # anti-aliased stride
            Ho, Wo = H // blk.stride, W // blk.stride
        identity = x
        if blk.downsample is not None:
            idn = ops.avgpool_nhwc(x, B, H, W, Cin, blk.stride) if blk.stride > 1 else x
            dsc, dsh = self._bn_affine(key + ".d", blk.downsample["1"])
            identity = ops.gemm_bn(idn, self._w1x1(key + ".d", blk.downsample["0"]), dsc, dsh, relu=False)
        sc, sh = self._bn_affine(key + ".3", blk.bn3)
        out = ops.gemm_bn_res_relu(out, self._w1x1(key + ".3", blk.conv3), sc, sh, identity)  # relu(bn3(conv3(out)) + identity), one launch
        return out, Ho, Wo, planes * 4

    def forward(self, x):
        R = self.input_resolution
        if x.dim() != 4 or x.shape[1] != 3 or x.shape[2] != R or x.shape[3] != R:
            raise PclipError(f"expected images [B,3,{R},{R}], got {tuple(x.shape)}")
        outs = [self._forward_chunk(x[i:i + self.chunk]) for i in range(0, x.shape[0], self.chunk)]
        return outs[0] if len(outs) == 1 else torch.cat(outs, dim=0)

    def _forward_chunk(self, img):
        B, R = img.shape[0], self.input_resolution
        w2 = self.conv1.weight.shape[0]
        if ops.stem_conv_applies(R, w2) and img.dtype in (torch.float32, torch.float16):
            # stem conv1 + bn1 + relu straight from the NCHW images (fp32 rounded to fp16 on the way): no cast pass, no im2col matrix
            sc, sh = self._bn_affine("s1", self.bn1)
            x = ops.stem_conv_bn(img, self._w3x3("s1", self.conv1), sc, sh, relu=True)
        else:
            if img.dtype == torch.float32:
                img = ops.cast_f16(img)
            img = img.contiguous()
            # stem (clip/model.py:138-142): the NCHW image is read through its strides by the first im2col
            x = self._conv3_bn_relu("s1", img, (3 * R * R, R, 1, R * R), B, R, R, 3, self.conv1, self.bn1, stride=2)
        H = W = (R - 1) // 2 + 1
        x = self._conv3_bn_relu("s2", x, (H * W * w2, W * w2, w2, 1), B, H, W, w2, self.conv2, self.bn2)
        C = self.conv3.weight.shape[0]
        if ops.conv3x3_pool_applies(H, W, w2, C):           # conv3 + bn3 + relu + avgpool(2) in one launch (the same bits)
            sc, sh = self._bn_affine("s3", self.bn3)
            x = ops.conv3x3_bn_pool(x, self._w3x3("s3", self.conv3), sc, sh, B, H, W, w2)
        else:
            x = self._conv3_bn_relu("s3", x, (H * W * w2, W * w2, w2, 1), B, H, W, w2, self.conv3, self.bn3)
            x = ops.avgpool_nhwc(x, B, H, W, C, 2)
        H, W = H // 2, W // 2
        for li in (1, 2, 3, 4):
            for bi, blk in enumerate(getattr(self, f"layer{li}")):
                x, H, W, C = self._bottleneck(f"l{li}.{bi}", blk, x, B, H, W, C)
        # attention pool (clip/model.py:67-92): q = k = v = tokens, separate projections, output of token 0
        ap = self.attnpool
        pos16 = self._cache.get("appos", ap.positional_embedding, lambda t: t.half().contiguous())
        wqkv = self._cache.get("apw", ap.q_proj.weight, lambda _: torch.cat([ap.q_proj.weight, ap.k_proj.weight, ap.v_proj.weight]).detach().contiguous())
        bqkv = self._cache.get("apb", ap.q_proj.bias, lambda _: torch.cat([ap.q_proj.bias, ap.k_proj.bias, ap.v_proj.bias]).detach().contiguous())
        L = H * W + 1
        tok = ops.attnpool_tokens(x, pos16, B, H * W, C)
        # only the pooled (mean) token's output is returned (clip/model.py:91 `x[0]`): project queries for token 0 only and
        # run a one-query attention per (image, head); keys / values still come from all HW + 1 tokens
        kv = ops.gemm(tok, wqkv[C:], bqkv[C:])
        q0 = ops.gemm(tok.view(B, L * C)[:, :C].contiguous(), wqkv[:C], bqkv[:C])
        a0 = ops.attention_first_queries(q0, kv, B, L, 1, self.heads)
        return ops.gemm(a0, ap.c_proj.weight, ap.c_proj.bias)


class CLIP(nn.Module):
    """clip/model.py:241-370 (transformer towers only)."""

    def __init__(self, embed_dim, image_resolution, vision_layers, vision_width, vision_patch_size, context_length,
                 vocab_size, transformer_width, transformer_heads, transformer_layers):
        super().__init__()
        self.context_length = context_length
        if isinstance(vision_layers, (tuple, list)):
            self.visual = ModifiedResNet(vision_layers, embed_dim, vision_width * 32 // 64, image_resolution, vision_width)
        else:
            self.visual = VisionTransformer(image_resolution, vision_patch_size, vision_width, vision_layers,
                                            vision_width // 64, embed_dim)
        self.transformer = _transformer(transformer_width, transformer_layers)
        self.transformer_heads = transformer_heads
        self.vocab_size = vocab_size
        self.token_embedding = _Box()
        self.token_embedding.weight = nn.Parameter(torch.empty(vocab_size, transformer_width), requires_grad=False)
        self.positional_embedding = nn.Parameter(torch.empty(context_length, transformer_width), requires_grad=False)
        self.ln_final = _ln(transformer_width)
        self.text_projection = nn.Parameter(torch.empty(transformer_width, embed_dim), requires_grad=False)
        self.logit_scale = nn.Parameter(torch.ones([]) * np.log(1 / 0.07), requires_grad=False)
        self._cache = _Cached()
        prefix = [("token_embedding.weight", self.token_embedding.weight), ("positional_embedding", self.positional_embedding)]
        head = [("ln_final.weight", self.ln_final.weight), ("ln_final.bias", self.ln_final.bias), ("text_projection", self.text_projection)]
        self.text_tower = Tower("encode_text", "text tower", "embeddings", blocks=self.transformer.resblocks, heads=transformer_heads, causal=True,
                                ln=self.ln_final, proj=self.text_projection, cache=self._cache, projT_key="tprojT", prefix=prefix, head=head,
                                pick=eot_row_pick)
        self.text_chunk = 1024

    @property
    def dtype(self):
        return self.visual.conv1.weight.dtype

    def encode_image(self, image):
        """[n, 3, R, R] -> [n, embed_dim] fp16 (clip/model.py:338-339).  A constant, unless grad mode is on and a parameter of the visual tower
        requires grad (`unfreeze`): then the tail of the tower from the first trainable block on is recorded for autograd (autograd.TowerTailFn;
        the same kernels, the same bits)."""
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.visual.parameters()):
            if isinstance(self.visual, ModifiedResNet):
                name = next(n for n, p in self.visual.named_parameters() if p.requires_grad)
                raise PclipError(f"encode_image: parameter visual.{name} requires grad, but the ModifiedResNet tower has no backward "
                                 "(only the transformer towers can be fine-tuned)")
            return self.visual(image)
        with torch.no_grad():
            return self.visual(image)

    def encode_text(self, text):
        """text [n, context_length] int64 -> [n, embed_dim] fp16 (clip/model.py:341-354).  Unlike the
        reference's per-class calls (utils.py:264-266, n = #templates) any n is efficient here."""
        plan = self.text_tower.tape_plan() if torch.is_grad_enabled() else (None, False)
        with torch.set_grad_enabled(plan[0] is not None):
            outs = [self._encode_text_chunk(text[i:i + self.text_chunk], plan) for i in range(0, text.shape[0], self.text_chunk)]
            return outs[0] if len(outs) == 1 else torch.cat(outs, dim=0)

    @property
    def _text_stem_opt_in(self):
        """unfreeze(stem=...) has opted the text prefix in: token_embedding / positional_embedding may train."""
        return self.text_tower.stem_opt_in

    @_text_stem_opt_in.setter
    def _text_stem_opt_in(self, value):
        self.text_tower.stem_opt_in = bool(value)

    def _text_tape_from(self):
        """As VisionTransformer._tape_from for the text tower (ln_final / text_projection are its heads)."""
        return self.text_tower.tape_from()

    def _text_tape_plan(self):
        """As VisionTransformer._tape_plan for the text tower."""
        return self.text_tower.tape_plan()

    def unfreeze(self, visual_blocks=0, text_blocks=0, heads=True, stem=False):
        """Make a tail of the transformer towers trainable: the last `visual_blocks` / `text_blocks` residual blocks and, with `heads`, ln_post / proj
        and ln_final / text_projection.  Returns the list of those parameters, ready for an optimizer; encode_image / encode_text then record their
        tail for autograd whenever grad mode is on.  Everything before the first trainable block stays frozen — unless `stem` opts a tower's prefix
        in: True (both towers), "visual" (conv1, class / positional embedding, ln_pre) or "text" (token / positional embedding).  Those parameters are
        then marked and returned too, the opt-in is recorded on the model, and a pass of that tower tapes the stem and every block (blocks that stay
        frozen pay for no weight gradient).  A prefix parameter that merely has requires_grad set, without this opt-in, is refused as before."""
        if stem not in (False, True, "visual", "text"):
            raise PclipError(f"unfreeze: stem={stem!r} is none of False, True, 'visual', 'text'")
        stem_visual, stem_text = stem in (True, "visual"), stem in (True, "text")
        if isinstance(self.visual, ModifiedResNet):                         # no backward: the tower stays frozen, the text side may train
            if visual_blocks:
                raise PclipError(f"unfreeze: visual_blocks={visual_blocks}, but the ModifiedResNet tower has no backward (only transformer towers)")
            if stem_visual:
                raise PclipError(f"unfreeze: stem={stem!r} asks for the visual stem, but the ModifiedResNet visual tower has no backward "
                                 "(only transformer towers; stem='text' trains the text embeddings beside it)")
            vis = []
        else:
            nv = len(self.visual.transformer.resblocks)
            if not 0 <= visual_blocks <= nv:
                raise PclipError(f"unfreeze: visual_blocks={visual_blocks} outside 0..{nv}")
            vis = [p for _, p in self.visual.tower.prefix] if stem_visual else []
            vis += [p for blk in list(self.visual.transformer.resblocks)[nv - visual_blocks:] for p in blk.parameters()]
            if heads:
                vis += [p for _, p in self.visual.tower.head]
        nt = len(self.transformer.resblocks)
        if not 0 <= text_blocks <= nt:
            raise PclipError(f"unfreeze: text_blocks={text_blocks} outside 0..{nt}")
        txt = [p for _, p in self.text_tower.prefix] if stem_text else []
        txt += [p for blk in list(self.transformer.resblocks)[nt - text_blocks:] for p in blk.parameters()]
        if heads:
            txt += [p for _, p in self.text_tower.head]
        if stem_visual:
            self.visual._stem_opt_in = True
        if stem_text:
            self._text_stem_opt_in = True
        params = vis + txt
        for p in params:
            p.requires_grad_(True)
        return params

    def _encode_text_chunk(self, text, plan=(None, False)):
        B, L = text.shape
        tw = self.text_tower
        if plan[1]:                                                              # whole-tower fine-tuning: the embedding and every block on the tape
            from ..autograd import TextEmbedFn
            x = TextEmbedFn.apply(text, self.token_embedding.weight, self.positional_embedding, self._cache)
        else:
            emb16 = self._cache.get("tok", self.token_embedding.weight, lambda t: t.half().contiguous())
            pos16 = self._cache.get("pos", self.positional_embedding, lambda t: t.half().contiguous())
            x = ops.text_embed(text, emb16, pos16)                               # 342-344
        return run_tower(tw, x, B, L, plan, tw.pick(B, L, x.device, text))       # 345-352

    def forward(self, image, text):
        """(logits_per_image [n_img, n_txt], logits_per_text = its transpose view), fp16 (clip/model.py:356-370): both feature matrices L2-normalised in fp16,
        the image side scaled by logit_scale.exp() and rounded, one cosine-logit kernel.  logit_scale stays fp32 under convert_weights, but as a 0-dim operand
        of an fp16 tensor the reference casts it to fp16 before the multiplication: the scale is the fp16-rounded value (14.2890625 for ln(1 / 0.07))."""
        with torch.no_grad():
            image_features = self.encode_image(image)
            text_features = self.encode_text(text)
            scale = float(self.logit_scale.exp().half())
            logits_per_image, _, _, _ = ops.cosine_logits(image_features, text_features, scale, normalize_a=True, normalize_b=True)
            logits_per_image = logits_per_image.contiguous()           # (dense as the reference's, whatever the prompt count: a copy only where n_txt % 8 != 0)
            return logits_per_image, logits_per_image.t()

    def contrastive_loss(self, image_features, text_features):
        """CLIP's symmetric contrastive loss of matching image / text features (the outputs of encode_image / encode_text, or trained copies of them) under
        this model's temperature: `utils.clip_contrastive_loss` with logit_scale.exp() in fp32 — NOT the fp16-rounded value `forward` reproduces.
        logit_scale is frozen by default; after `model.logit_scale.requires_grad_(True)` its gradient arrives through torch's own exp node.  Features of
        a frozen model are constants; after `unfreeze` (or `requires_grad_` on a tail of a tower) encode_image / encode_text record that tail, and this
        loss's feature gradients flow on through the blocks' backward kernels into the parameters' .grad."""
        from ..utils import clip_contrastive_loss
        return clip_contrastive_loss(image_features, text_features, self.logit_scale.float().exp())

    def sigmoid_loss(self, image_features, text_features, logit_bias, image_ids=None, text_ids=None):
        """SigLIP's pairwise sigmoid loss (`utils.clip_sigmoid_loss`) under this model's temperature, logit_scale.exp() in fp32: a pair is positive iff its ids
        agree (several images per class are several positives of that class's text); without ids the positives are the diagonal.  logit_bias is the
        CALLER's float or 0-dim tensor (SigLIP starts it at -10): the model keeps no such parameter, its state dict stays the reference's.  Gradients
        reach logit_scale, logit_bias and the unfrozen tails of the towers as under `contrastive_loss`."""
        from ..utils import clip_sigmoid_loss
        return clip_sigmoid_loss(image_features, text_features, self.logit_scale.float().exp(), logit_bias, image_ids, text_ids)


def convert_weights(model: nn.Module):
    """fp16 for Linear/conv/attention/projection parameters, fp32 elsewhere (clip/model.py:373-394)."""
    half_suffixes = ("in_proj_weight", "in_proj_bias", "out_proj.weight", "out_proj.bias", "c_fc.weight", "c_fc.bias",
                     "c_proj.weight", "c_proj.bias", "visual.proj", "text_projection", "q_proj.weight", "q_proj.bias",
                     "k_proj.weight", "k_proj.bias", "v_proj.weight", "v_proj.bias")
    for name, p in model.named_parameters():
        is_conv = p.dim() == 4                               # every nn.Conv2d weight (ViT patch conv, all ResNet convs)
        p.data = p.data.half() if (is_conv or name.endswith(half_suffixes)) else p.data.float()


def build_model(state_dict: dict):
    """Same shape inference as the reference's build_model (clip/model.py:397-434)."""
    if "visual.proj" in state_dict:
        vision_width = state_dict["visual.conv1.weight"].shape[0]
        vision_layers = len([k for k in state_dict if k.startswith("visual.") and k.endswith(".attn.in_proj_weight")])
        vision_patch_size = state_dict["visual.conv1.weight"].shape[-1]
        grid_size = round((state_dict["visual.positional_embedding"].shape[0] - 1) ** 0.5)
        image_resolution = vision_patch_size * grid_size
    else:
        vision_layers = tuple(len(set(k.split(".")[2] for k in state_dict if k.startswith(f"visual.layer{b}"))) for b in (1, 2, 3, 4))
        vision_width = state_dict["visual.layer1.0.conv1.weight"].shape[0]
        output_width = round((state_dict["visual.attnpool.positional_embedding"].shape[0] - 1) ** 0.5)
        vision_patch_size = None
        assert output_width ** 2 + 1 == state_dict["visual.attnpool.positional_embedding"].shape[0]
        image_resolution = output_width * 32
    embed_dim = state_dict["text_projection"].shape[1]
    context_length = state_dict["positional_embedding"].shape[0]
    vocab_size = state_dict["token_embedding.weight"].shape[0]
    transformer_width = state_dict["ln_final.weight"].shape[0]
    transformer_heads = transformer_width // 64
    transformer_layers = len(set(k.split(".")[2] for k in state_dict if k.startswith("transformer.resblocks")))
    model = CLIP(embed_dim, image_resolution, vision_layers, vision_width, vision_patch_size, context_length,
                 vocab_size, transformer_width, transformer_heads, transformer_layers)
    sd = OrderedDict((k, v) for k, v in state_dict.items() if k not in ("input_resolution", "context_length", "vocab_size"))
    convert_weights(model)
    model.load_state_dict(sd)
    convert_weights(model)
    return model.eval()


# Backbone hyper-parameters OpenAI's checkpoints resolve to.
BACKBONES = {
    "ViT-B/32": dict(embed_dim=512, image_resolution=224, vision_layers=12, vision_width=768, vision_patch_size=32,
                     context_length=77, vocab_size=49408, transformer_width=512, transformer_heads=8, transformer_layers=12),
    "ViT-B/16": dict(embed_dim=512, image_resolution=224, vision_layers=12, vision_width=768, vision_patch_size=16,
                     context_length=77, vocab_size=49408, transformer_width=512, transformer_heads=8, transformer_layers=12),
    "RN50": dict(embed_dim=1024, image_resolution=224, vision_layers=(3, 4, 6, 3), vision_width=64, vision_patch_size=None,
                 context_length=77, vocab_size=49408, transformer_width=512, transformer_heads=8, transformer_layers=12),
    "RN101": dict(embed_dim=512, image_resolution=224, vision_layers=(3, 4, 23, 3), vision_width=64, vision_patch_size=None,
                  context_length=77, vocab_size=49408, transformer_width=512, transformer_heads=8, transformer_layers=12),
    "ViT-L/14": dict(embed_dim=768, image_resolution=224, vision_layers=24, vision_width=1024, vision_patch_size=14,
                     context_length=77, vocab_size=49408, transformer_width=768, transformer_heads=12, transformer_layers=12),
    # OpenAI's wide ResNets (the reference's RN50x4.pt / RN50x16.pt): 80 / 96-wide stems, 288 / 384 px, attention pools of 82 / 145 tokens
    "RN50x4": dict(embed_dim=640, image_resolution=288, vision_layers=(4, 6, 10, 6), vision_width=80, vision_patch_size=None,
                   context_length=77, vocab_size=49408, transformer_width=640, transformer_heads=10, transformer_layers=12),
    "RN50x16": dict(embed_dim=768, image_resolution=384, vision_layers=(6, 8, 18, 8), vision_width=96, vision_patch_size=None,
                    context_length=77, vocab_size=49408, transformer_width=768, transformer_heads=12, transformer_layers=12),
    # OpenAI's ViT-L-14-336px.pt (not in the reference's download list: load it by path; 24 x 24 patches + 1 = 577 tokens)
    "ViT-L/14@336px": dict(embed_dim=768, image_resolution=336, vision_layers=24, vision_width=1024, vision_patch_size=14,
                           context_length=77, vocab_size=49408, transformer_width=768, transformer_heads=12, transformer_layers=12),
}


def random_state_dict(seed: int = 1, **kw) -> "OrderedDict[str, torch.Tensor]":
    """Seeded random-init weights with the statistics of CLIP.initialize_parameters
    (clip/model.py:297-324) — there are no pretrained checkpoints in the build environment."""
    g = torch.Generator().manual_seed(seed)
    Wt, Lt, E = kw["transformer_width"], kw["transformer_layers"], kw["embed_dim"]
    rn = lambda *shape, std=1.0: torch.randn(*shape, generator=g) * std
    sd = OrderedDict()
    if isinstance(kw["vision_layers"], (tuple, list)):
        w = kw["vision_width"]

        def conv(name, co, ci, k):
            sd[name + ".weight"] = rn(co, ci, k, k, std=(ci * k * k) ** -0.5)

        def bn(name, ch, gamma=1.0):
            sd[name + ".weight"] = gamma * (1 + rn(ch, std=0.05))
            sd[name + ".bias"] = rn(ch, std=0.05)
            sd[name + ".running_mean"] = rn(ch, std=0.1)
            sd[name + ".running_var"] = 1 + 0.2 * torch.rand(ch, generator=g)
            sd[name + ".num_batches_tracked"] = torch.tensor(0, dtype=torch.long)

        conv("visual.conv1", w // 2, 3, 3); bn("visual.bn1", w // 2)
        conv("visual.conv2", w // 2, w // 2, 3); bn("visual.bn2", w // 2)
        conv("visual.conv3", w, w // 2, 3); bn("visual.bn3", w)
        inpl = w
        for li, (planes, nblk, stride) in enumerate(zip((w, 2 * w, 4 * w, 8 * w), kw["vision_layers"], (1, 2, 2, 2)), 1):
            for bi in range(nblk):
                p = f"visual.layer{li}.{bi}."
                st = stride if bi == 0 else 1
                conv(p + "conv1", planes, inpl, 1); bn(p + "bn1", planes)
                conv(p + "conv2", planes, planes, 3); bn(p + "bn2", planes)
                conv(p + "conv3", planes * 4, planes, 1); bn(p + "bn3", planes * 4, gamma=0.5)
                if st > 1 or inpl != planes * 4:
                    conv(p + "downsample.0", planes * 4, inpl, 1); bn(p + "downsample.1", planes * 4)
                inpl = planes * 4
        emb = w * 32
        sd["visual.attnpool.positional_embedding"] = rn((kw["image_resolution"] // 32) ** 2 + 1, emb, std=emb ** -0.5)
        for nm in ("k_proj", "q_proj", "v_proj"):
            sd[f"visual.attnpool.{nm}.weight"] = rn(emb, emb, std=emb ** -0.5)
            sd[f"visual.attnpool.{nm}.bias"] = rn(emb, std=0.02)
        sd["visual.attnpool.c_proj.weight"] = rn(E, emb, std=emb ** -0.5)
        sd["visual.attnpool.c_proj.bias"] = rn(E, std=0.02)
    else:
        W, Lv, P = kw["vision_width"], kw["vision_layers"], kw["vision_patch_size"]
        G = kw["image_resolution"] // P
        sd["visual.class_embedding"] = rn(W, std=W ** -0.5)
        sd["visual.positional_embedding"] = rn(G * G + 1, W, std=W ** -0.5)
        sd["visual.proj"] = rn(W, E, std=W ** -0.5)
        sd["visual.conv1.weight"] = rn(W, 3, P, P, std=(3 * P * P) ** -0.5)
        for nm in ("ln_pre", "ln_post"):
            sd[f"visual.{nm}.weight"] = 1 + rn(W, std=0.02)
            sd[f"visual.{nm}.bias"] = rn(W, std=0.02)

    def blocks(prefix, width, layers):
        proj_std, attn_std, fc_std = (width ** -0.5) * ((2 * layers) ** -0.5), width ** -0.5, (2 * width) ** -0.5
        for i in range(layers):
            p = f"{prefix}resblocks.{i}."
            sd[p + "attn.in_proj_weight"] = rn(3 * width, width, std=attn_std)
            sd[p + "attn.in_proj_bias"] = rn(3 * width, std=0.02)
            sd[p + "attn.out_proj.weight"] = rn(width, width, std=proj_std)
            sd[p + "attn.out_proj.bias"] = rn(width, std=0.02)
            sd[p + "ln_1.weight"] = 1 + rn(width, std=0.02)
            sd[p + "ln_1.bias"] = rn(width, std=0.02)
            sd[p + "mlp.c_fc.weight"] = rn(4 * width, width, std=fc_std)
            sd[p + "mlp.c_fc.bias"] = rn(4 * width, std=0.02)
            sd[p + "mlp.c_proj.weight"] = rn(width, 4 * width, std=proj_std)
            sd[p + "mlp.c_proj.bias"] = rn(width, std=0.02)
            sd[p + "ln_2.weight"] = 1 + rn(width, std=0.02)
            sd[p + "ln_2.bias"] = rn(width, std=0.02)

    if not isinstance(kw["vision_layers"], (tuple, list)):
        blocks("visual.transformer.", kw["vision_width"], kw["vision_layers"])
    blocks("transformer.", Wt, Lt)
    sd["token_embedding.weight"] = rn(kw["vocab_size"], Wt, std=0.02)
    sd["positional_embedding"] = rn(kw["context_length"], Wt, std=0.01)
    sd["ln_final.weight"] = 1 + rn(Wt, std=0.02)
    sd["ln_final.bias"] = rn(Wt, std=0.02)
    sd["text_projection"] = rn(Wt, E, std=Wt ** -0.5)
    sd["logit_scale"] = torch.ones([]) * np.log(1 / 0.07)
    return sd
