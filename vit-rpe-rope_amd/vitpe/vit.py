"""Drop-in mirror of the reference's models/vit.py: same constructor, attribute names and
state_dict key set (incl. the aliased `blocks.i.attn.pos_encoding.*` keys);
forward dispatches to the `torch.ops.vitpe.*` custom ops (HIP kernels).  Inputs must live on
the HIP device: there is no CPU path.

Extension over the reference: `model.set_compute_dtype(torch.bfloat16)` switches activations
and GEMM operands to bf16 (fp32 accumulate); the default float32 uses exact-fp32 MFMA and is
the mode the 1e-4 parity gate runs in.
"""
import contextlib
import math

import torch
import torch.nn as nn

from . import kernels as K
from . import ops  # noqa: F401  (registers torch.ops.vitpe.*)
from ._lib import VitpeError, require_device
from .positional_encoding import (AbsolutePositionalEncoding, NoPositionalEncoding, PolynomialRPE,
                                  RelativePositionalEncoding, RoPEAxial, RoPEMixed, _MixedTables)

_MODE = {"none": 0, "absolute": 1, "relative": 2, "polynomial": 3, "rope-axial": 4, "rope-mixed": 5}


def _check_rate(name, p):
    if not 0.0 <= float(p) < 1.0:
        raise ValueError(f"vitpe: {name} must be in [0, 1), got {p}")
    return float(p)


def _pe_args(pe, use_rope_tables: bool):
    """(mode, pe_param, inv_freq, degree, per_head) for torch.ops.vitpe.attention."""
    if isinstance(pe, RelativePositionalEncoding):
        return _MODE["relative"], pe.relative_position_bias_table, None, 0, False
    if isinstance(pe, PolynomialRPE):
        return _MODE["polynomial"], pe.coefficients, None, pe.degree, not pe.shared_across_heads
    if isinstance(pe, RoPEAxial) and use_rope_tables:
        return _MODE["rope-axial"], None, pe.inv_freq, 0, False
    if isinstance(pe, RoPEMixed) and use_rope_tables:
        return _MODE["rope-mixed"], pe.freqs, None, 0, False
    return _MODE["none"], None, None, 0, False


class Mlp(nn.Module):
    """fc1 -> GELU(erf) -> fc2, the arithmetic of timm's Mlp as the reference instantiates it
    (vit.py:118; third-party, parity unpinned).  Same state_dict keys (fc1.*, fc2.*).  drop > 0 in training: fc1 -> GELU ->
    dropout -> fc2 -> dropout (timm's drop1 / drop2 order) on the dropout kernels; `last_rng` ([2, 2] int64 device tensor)
    then holds the (seed, offset) pairs the last forward drew for drop1 (row 0) and drop2 (row 1), None if it drew none."""

    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, drop=0.):
        super().__init__()
        if act_layer is not nn.GELU:
            raise NotImplementedError("vitpe Mlp: only act_layer=nn.GELU (the reference's configuration)")
        out_features = out_features or in_features
        hidden_features = hidden_features or in_features
        self.fc1 = nn.Linear(in_features, hidden_features)
        self.act = act_layer()
        self.fc2 = nn.Linear(hidden_features, out_features)
        self.drop = _check_rate("drop", drop)
        self.last_rng = None

    def forward(self, x, resid=None):
        require_device(x)
        if self.training and self.drop > 0.:
            self.last_rng = K.new_rng_pairs(2, x.device)
            return torch.ops.vitpe.mlp(x, self.fc1.weight, self.fc1.bias, self.fc2.weight, self.fc2.bias, resid,
                                       self.drop, self.last_rng)[0]
        self.last_rng = None   # (no pairs drawn by this forward)
        return torch.ops.vitpe.mlp(x, self.fc1.weight, self.fc1.bias, self.fc2.weight, self.fc2.bias, resid)[0]


class Attention(nn.Module):
    """reference vit.py:14-98; forward(x, freqs_cis=None) returns proj(attention(x)).

    qkv_bias, or a non-zero attn_drop / proj_drop in training, takes the qkv Linear (bias epilogue) + attention core route
    (the one-kernel fused paths have neither a bias input nor dropout); attn_drop runs inside the core kernel, proj_drop
    as the elementwise dropout kernel.  In eval mode, or with zero rates, the dropout kernels are not launched.  `last_rng`
    ([2, 2] int64 device tensor) holds the (seed, offset) pairs the last forward drew (None if it drew none) for the attention-probability
    site (row 0) and the proj site (row 1).  The one refused combination: gradients of caller-supplied rotary tables
    together with attn_drop > 0 (NotImplementedError)."""

    def __init__(self, dim, num_heads=8, qkv_bias=False, attn_drop=0., proj_drop=0.):
        super().__init__()
        self.attn_drop_p = _check_rate("attn_drop", attn_drop)
        self.proj_drop_p = _check_rate("proj_drop", proj_drop)
        self.last_rng = None
        self.num_heads = num_heads
        self.head_dim = dim // num_heads
        self.scale = self.head_dim ** -0.5
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.attn_drop = nn.Dropout(attn_drop)
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = nn.Dropout(proj_drop)
        self.pos_encoding = None

    def _pe_operands(self, N, freqs_cis):
        """(mode, pe_param, inv_freq, degree, per_head, cos, sin, tables_grad): the positional-encoding arguments of the
        attention ops for N tokens and the caller's freqs_cis."""
        # RoPE rotates only when the caller passes freqs_cis (reference vit.py:51).  VisionTransformer.forward_features
        # passes a marker and the kernel builds the tables on the device from the module's own parameters (which keeps
        # the RoPE-mixed frequencies trainable).  The caller-table rule (vit.py:51): a caller's own (cos, sin) tensors are
        # used as given, with their own shape ([P, hd/2] or [H, P, hd/2], vit.py:53-64), when and only when
        # self.pos_encoding is a RoPEAxial / RoPEMixed.  Under every other encoding (None, none, absolute, relative,
        # polynomial) the reference takes its else branch (vit.py:73-81): freqs_cis is never looked at -- nothing is
        # rotated, no shape is checked -- and the relative / polynomial bias is still added.
        mode, pe_param, inv_freq, degree, per_head = _pe_args(self.pos_encoding, freqs_cis is not None)
        cos = sin = None
        tables_grad = False
        if isinstance(self.pos_encoding, (RoPEAxial, RoPEMixed)) and isinstance(freqs_cis, (tuple, list)) \
                and len(freqs_cis) == 2 and all(torch.is_tensor(t) for t in freqs_cis):
            cos, sin = freqs_cis
            if not (cos.is_cuda and sin.is_cuda):
                raise VitpeError("vitpe: HIP device tensor required (got a CPU tensor; there is no CPU fallback)")
            if cos.shape != sin.shape or cos.dim() not in (2, 3) or tuple(cos.shape[-2:]) != (N - 1, self.head_dim // 2) \
                    or (cos.dim() == 3 and cos.shape[0] != self.num_heads):
                # (reshape_for_broadcast's error, reference rope_utils.py:39-66)
                raise ValueError(f"Unexpected shape for freqs_cis: {tuple(cos.shape)}")
            if (cos.requires_grad or sin.requires_grad) and self._own_mixed_tables(cos, sin):
                # RoPEMixed.get_freqs_cis of this module's own frequencies (reference vit.py:262-266): the kernel
                # rebuilds the tables from the parameter and sends the gradient there, as the reference's autograd would
                cos = sin = None
            else:
                # constant tables, or differentiable ones from anywhere else: used as given; the latter take the
                # qkv Linear + core route, whose backward returns d cos / d sin (vitpe::attention, tables_grad)
                tables_grad = torch.is_grad_enabled() and (cos.requires_grad or sin.requires_grad)
                mode, pe_param, inv_freq = (_MODE["rope-axial"] if cos.dim() == 2 else _MODE["rope-mixed"]), None, None
        return mode, pe_param, inv_freq, degree, per_head, cos, sin, tables_grad

    def forward(self, x, freqs_cis=None, resid=None):
        require_device(x)
        B, N, C = x.shape
        mode, pe_param, inv_freq, degree, per_head, cos, sin, tables_grad = self._pe_operands(N, freqs_cis)
        grid = int(math.sqrt(N - 1))
        attn_p = self.attn_drop_p if self.training else 0.
        proj_p = self.proj_drop_p if self.training else 0.
        self.last_rng = None   # (set below if this forward draws pairs)
        if self.qkv.bias is None and attn_p == 0. and proj_p == 0.:
            y, _, _ = torch.ops.vitpe.attention(x, self.qkv.weight, self.proj.weight, self.proj.bias, resid, self.num_heads,
                                             mode, grid, pe_param, inv_freq, degree, per_head, cos, sin, tables_grad)
            return y
        if tables_grad and attn_p > 0.:
            raise NotImplementedError("vitpe Attention: gradients of caller-supplied rotary tables together with "
                                      "attn_drop > 0 (pass constant tables, or set attn_drop=0)")
        rng = None
        if attn_p > 0. or proj_p > 0.:
            rng = self.last_rng = K.new_rng_pairs(2, x.device)
        y, _, _ = torch.ops.vitpe.attention_drop(x, self.qkv.weight, self.qkv.bias, self.proj.weight, self.proj.bias, resid,
                                              self.num_heads, mode, grid, pe_param, inv_freq, degree, per_head, cos, sin,
                                              tables_grad, attn_p, proj_p, rng)
        return y

    def attention_probs(self, x, freqs_cis=None, cls_only=False):
        """The attention probabilities of forward(x, freqs_cis): softmax(QK^T hd^-0.5 [+ bias]), the reference's `attn`
        after .softmax(dim=-1) and before attn_drop (vit.py:71-84) -- what a forward hook on its softmax would catch.
        x: the same input as forward's (the tokens after norm1); freqs_cis: the same marker or (cos, sin) tables.
        -> fp32 [B, H, N, N]; cls_only: the class token's row alone, [B, H, N].

        Always the undropped softmax, whatever self.training and attn_drop are; no RNG is drawn; the result carries no
        gradient.  The route is the qkv Linear (with qkv.bias if the module has one) + the probabilities kernel of the
        attention core at every geometry -- also at those where forward runs a one-kernel fused path (N 65 / hd 32,
        N 197 / hd 64), which keep the probabilities on the chip."""
        require_device(x)
        B, N, C = x.shape
        with torch.no_grad():
            mode, pe_param, inv_freq, degree, per_head, cos, sin, _ = self._pe_operands(N, freqs_cis)
            qkv = K.linear(x.contiguous().view(B * N, C), ops._shadow(self.qkv.weight, x.dtype), self.qkv.bias).view(B, N, 3 * C)
            return torch.ops.vitpe.attention_probs(qkv, self.num_heads, mode, int(math.sqrt(N - 1)), pe_param, inv_freq,
                                                   degree, per_head, cos, sin, bool(cls_only))

    def attention_stats(self, x, freqs_cis=None, weights=None, unit=1.0):
        """Statistics of attention_probs(x, freqs_cis), reduced inside the kernel -- the [N, N] maps are never stored
        (kernels.attention_core_stats).  -> (stats fp32 [B, H, 4], colsum): the slots kernels.STAT_DISTANCE (mean attention
        distance on the sqrt(N - 1)-wide token raster, in units of `unit`), STAT_ENTROPY, STAT_CLS_MASS, STAT_CLS_ENTROPY;
        weights fp32 [B, N]: colsum fp32 [B, H, N] = sum_i weights[b, i] p_ij (what attention rollout needs), else None.

        As attention_probs: the module's own rotation and bias handling, the qkv Linear (with qkv.bias if the module has one)
        + the statistics kernel of the attention core at every geometry; always the undropped softmax, no RNG drawn, no
        gradient."""
        require_device(x, weights)
        B, N, C = x.shape
        with torch.no_grad():
            mode, pe_param, inv_freq, degree, per_head, cos, sin, _ = self._pe_operands(N, freqs_cis)
            qkv = K.linear(x.contiguous().view(B * N, C), ops._shadow(self.qkv.weight, x.dtype), self.qkv.bias).view(B, N, 3 * C)
            t = ops._pe_tables(mode, int(math.sqrt(N - 1)), pe_param, inv_freq, degree, per_head, cos, sin)
            return K.attention_core_stats(qkv, self.num_heads, t, unit=unit, weights=weights)

    def attention_relevance(self, x, dy, freqs_cis=None, weights=None, clamp=True):
        """One step of the gradient-weighted attention relevance (Chefer, Gur & Wolf, ICCV 2021) of forward(x, freqs_cis),
        reduced inside the kernel -- neither the [N, N] probabilities A nor their gradient G is stored
        (kernels.attention_core_relevance).  x: forward's input; dy [B, N, C]: the gradient of a scalar w.r.t. forward's
        output (x's dtype); weights fp32 [B, N], default e_cls (1 on the class token).
        -> colsum fp32 [B, H, N] = sum_i weights[b, i] f(G_ij A_ij) with G = dO_h V_h^T, dO = dy W_proj the gradient w.r.t. the
        merged-head output in front of proj (the proj bias plays no part), V the head's value rows of the qkv projection
        (unrotated, with qkv.bias if the module has one), f = max(0, .) under clamp and the identity without.

        As attention_stats: the module's own rotation and bias handling, the qkv Linear + the relevance kernel of the
        attention core at every geometry it fits; always the undropped softmax, no RNG drawn, no gradient."""
        require_device(x, dy, weights)
        B, N, C = x.shape
        if tuple(dy.shape) != (B, N, C) or dy.dtype != x.dtype:
            raise VitpeError(f"vitpe attention_relevance: dy must be {x.dtype} {(B, N, C)}")
        with torch.no_grad():
            mode, pe_param, inv_freq, degree, per_head, cos, sin, _ = self._pe_operands(N, freqs_cis)
            qkv = K.linear(x.contiguous().view(B * N, C), ops._shadow(self.qkv.weight, x.dtype), self.qkv.bias).view(B, N, 3 * C)
            dout = K.linear(dy.contiguous().view(B * N, C), ops._shadow_t(self.proj.weight, x.dtype), None).view(B, N, C)
            t = ops._pe_tables(mode, int(math.sqrt(N - 1)), pe_param, inv_freq, degree, per_head, cos, sin)
            if weights is None:
                weights = torch.zeros(B, N, dtype=torch.float32, device=x.device)
                weights[:, 0] = 1.0
            return K.attention_core_relevance(qkv, dout, self.num_heads, t, weights, clamp=clamp)

    def _own_mixed_tables(self, cos, sin):
        """Are (cos, sin) provably RoPEMixed.get_freqs_cis of this module's own `freqs` (one _MixedTables node whose
        input is the parameter itself)?"""
        pe = self.pos_encoding
        fn = cos.grad_fn
        if not isinstance(pe, RoPEMixed) or fn is None or sin.grad_fn is not fn \
                or type(fn) is not _MixedTables._backward_cls:
            return False
        src = fn.next_functions[0][0] if fn.next_functions else None
        return src is not None and getattr(src, "variable", None) is pe.freqs

    def set_pos_encoding(self, pos_encoding):
        self.pos_encoding = pos_encoding


class Block(nn.Module):
    """Pre-LN residual block; reference vit.py:100-129."""

    def __init__(self, dim, num_heads, mlp_ratio=4., qkv_bias=False, drop=0., attn_drop=0.,
                 drop_path=0., act_layer=nn.GELU, norm_layer=nn.LayerNorm):
        super().__init__()
        if norm_layer is not nn.LayerNorm:
            raise NotImplementedError("vitpe Block: nn.LayerNorm only (as the reference builds it)")
        self.norm1 = norm_layer(dim)
        self.attn = Attention(dim, num_heads=num_heads, qkv_bias=qkv_bias, attn_drop=attn_drop, proj_drop=drop)
        # stochastic depth (reference vit.py:115: timm DropPath, scale_by_keep=True -- third-party, parity unpinned): one
        # keep decision per sample for each branch, on the drop-path kernel with the residual fused.  No parameters, so
        # nn.Identity keeps the reference's attribute and state_dict surface; the rate lives in drop_path_p.
        self.drop_path = nn.Identity()
        self.drop_path_p = _check_rate("drop_path", drop_path)
        self.last_rng = None   # [2, 2] int64: the pairs of the attention branch (row 0) and the MLP branch (row 1)
        self.norm2 = norm_layer(dim)
        self.mlp = Mlp(in_features=dim, hidden_features=int(dim * mlp_ratio), act_layer=act_layer, drop=drop)

    def forward(self, x, freqs_cis=None):
        n1 = torch.ops.vitpe.layer_norm(x, self.norm1.weight, self.norm1.bias, self.norm1.eps)[0]
        if self.training and self.drop_path_p > 0.:
            rng = self.last_rng = K.new_rng_pairs(2, x.device)
            x = torch.ops.vitpe.drop_path(self.attn(n1, freqs_cis=freqs_cis), x, self.drop_path_p, rng[0])
            n2 = torch.ops.vitpe.layer_norm(x, self.norm2.weight, self.norm2.bias, self.norm2.eps)[0]
            return torch.ops.vitpe.drop_path(self.mlp(n2), x, self.drop_path_p, rng[1])
        self.last_rng = None   # (no pairs drawn by this forward)
        x = self.attn(n1, freqs_cis=freqs_cis, resid=x)      # x + attn(norm1(x)), residual fused in the proj GEMM
        n2 = torch.ops.vitpe.layer_norm(x, self.norm2.weight, self.norm2.bias, self.norm2.eps)[0]
        return self.mlp(n2, resid=x)                          # x + mlp(norm2(x)), residual fused in the fc2 GEMM

    def attention_probs(self, x, freqs_cis=None, cls_only=False):
        """The attention probabilities of this block's forward(x, freqs_cis): Attention.attention_probs on norm1(x)."""
        with torch.no_grad():
            n1 = torch.ops.vitpe.layer_norm(x, self.norm1.weight, self.norm1.bias, self.norm1.eps)[0]
        return self.attn.attention_probs(n1, freqs_cis=freqs_cis, cls_only=cls_only)

    def attention_stats(self, x, freqs_cis=None, weights=None, unit=1.0):
        """The attention statistics of this block's forward(x, freqs_cis): Attention.attention_stats on norm1(x)."""
        require_device(x, weights)
        with torch.no_grad():
            n1 = torch.ops.vitpe.layer_norm(x, self.norm1.weight, self.norm1.bias, self.norm1.eps)[0]
        return self.attn.attention_stats(n1, freqs_cis=freqs_cis, weights=weights, unit=unit)

    def attention_relevance(self, x, dmid, freqs_cis=None, weights=None, clamp=True):
        """The relevance step of this block's forward(x, freqs_cis): Attention.attention_relevance on norm1(x).  dmid: the
        gradient at the block's x + attn(norm1(x)), which is the gradient of the attention branch's output."""
        require_device(x, dmid, weights)
        with torch.no_grad():
            n1 = torch.ops.vitpe.layer_norm(x, self.norm1.weight, self.norm1.bias, self.norm1.eps)[0]
        return self.attn.attention_relevance(n1, dmid, freqs_cis=freqs_cis, weights=weights, clamp=clamp)

    def set_pos_encoding(self, pos_encoding):
        self.attn.set_pos_encoding(pos_encoding)


class VisionTransformer(nn.Module):
    """reference vit.py:131-285, constructor kept verbatim (vit.py:148-151); keyword-only extras behind it: qkv_bias,
    drop_rate (proj and Mlp dropout), attn_drop_rate, drop_path_rate (stochastic depth, rising linearly from 0 at the first
    block to drop_path_rate at the last) -- what the reference's Block accepts but its VisionTransformer never passes."""

    def __init__(self, img_size=32, patch_size=4, in_chans=3, num_classes=10,
                 embed_dim=192, depth=6, num_heads=6, mlp_ratio=4.,
                 pos_encoding='absolute', rope_theta=100.0,
                 poly_degree=3, poly_shared_heads=True, *,
                 qkv_bias=False, drop_rate=0., attn_drop_rate=0., drop_path_rate=0.):
        super().__init__()
        self.qkv_bias = bool(qkv_bias)
        self.drop_rate = _check_rate("drop_rate", drop_rate)
        self.attn_drop_rate = _check_rate("attn_drop_rate", attn_drop_rate)
        self.drop_path_rate = _check_rate("drop_path_rate", drop_path_rate)
        self.num_classes = num_classes
        self.embed_dim = embed_dim
        self.patch_size = patch_size
        self.pos_encoding_type = pos_encoding
        self.head_dim = embed_dim // num_heads
        self.num_heads = num_heads
        self.num_patches = (img_size // patch_size) ** 2
        self.compute_dtype = torch.float32

        # kept as nn.Conv2d for the state_dict surface (weight [d,C,p,p]); executed as unfold + GEMM
        self.patch_embed = nn.Conv2d(in_chans, embed_dim, kernel_size=patch_size, stride=patch_size)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))

        self.use_pos_embed_in_forward = False
        self.use_rope = False
        if pos_encoding == 'absolute':
            self.pos_embed = AbsolutePositionalEncoding(embed_dim)
            self.use_pos_embed_in_forward = True
        elif pos_encoding == 'relative':
            self.pos_embed = RelativePositionalEncoding(self.num_patches, num_heads)
        elif pos_encoding == 'polynomial':
            self.pos_embed = PolynomialRPE(self.num_patches, degree=poly_degree, num_heads=num_heads,
                                           shared_across_heads=poly_shared_heads)
        elif pos_encoding == 'rope-axial':
            self.pos_embed = RoPEAxial(dim=self.head_dim, theta=rope_theta)
            self.use_rope = True
        elif pos_encoding == 'rope-mixed':
            self.pos_embed = RoPEMixed(dim=self.head_dim, num_heads=num_heads, theta=rope_theta)
            self.use_rope = True
        elif pos_encoding == 'none':
            self.pos_embed = NoPositionalEncoding()
        else:
            raise ValueError(f"Unknown positional encoding type: {pos_encoding}")

        dpr = [self.drop_path_rate * i / max(depth - 1, 1) for i in range(depth)]
        self.blocks = nn.ModuleList([Block(embed_dim, num_heads, mlp_ratio, qkv_bias=self.qkv_bias, drop=self.drop_rate,
                                           attn_drop=self.attn_drop_rate, drop_path=dpr[i]) for i in range(depth)])
        if not self.use_pos_embed_in_forward:
            for block in self.blocks:  # ONE shared PE module, registered in every block (vit.py:205-207)
                block.set_pos_encoding(self.pos_embed)

        self.norm = nn.LayerNorm(embed_dim)
        self.head = nn.Linear(embed_dim, num_classes)
        self.apply(self._init_weights)

    def _init_weights(self, m):
        """reference vit.py:216-233."""
        if isinstance(m, nn.Linear):
            nn.init.trunc_normal_(m.weight, std=0.02)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.LayerNorm):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)
        elif isinstance(m, nn.Conv2d):
            nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)

    def set_compute_dtype(self, dtype):
        if dtype not in (torch.float32, torch.bfloat16):
            raise VitpeError("compute dtype must be torch.float32 or torch.bfloat16")
        self.compute_dtype = dtype
        return self

    def saliency(self, images, target=None):
        """d logits[b, target_b] / d images[b] -> fp32 [B, C, S, S].  target: LongTensor [B], or None = the arg-max class
        of each image.  Eval semantics (no dropout, no stochastic depth, no RNG drawn; the training flags are restored
        afterwards).  The tokens the patch embed leaves are the leaf: torch.autograd.grad(..., inputs=[tokens]) gives
        d tokens through the blocks' own backward, and the patch-embed data-gradient kernel (kernels.patch_embed_dgrad,
        vitpe_patch_embed_dgrad) folds it onto the pixels.  No parameter's .grad is created or changed, `images` is left
        as it is, and the result carries no graph (no second derivatives).  vitpe::patch_embed itself still returns no
        gradient for `images`: forward keeps refusing images that require grad."""
        require_device(images)
        B, C, H, W = images.shape
        if H != W:
            raise VitpeError("vitpe saliency: square images")
        flags = [(m, m.training) for m in self.modules()]
        self.eval()
        try:
            with torch.no_grad():
                tok = self._embed(images.detach())
            with torch.enable_grad():
                tok = tok.requires_grad_(True)
                logits = self._head(self._blocks(tok, (H // self.patch_size) * (W // self.patch_size)))
                if target is None:
                    target = logits.detach().argmax(dim=1)
                elif target.dtype != torch.int64 or tuple(target.shape) != (B,):
                    raise ValueError("vitpe saliency: target must be a LongTensor [B]")
                picked = logits.gather(1, target.to(logits.device).view(-1, 1)).sum()
                (dtok,) = torch.autograd.grad(picked, inputs=[tok])
            with torch.no_grad():
                w = ops._shadow(self.patch_embed.weight.detach().reshape(self.embed_dim, -1), self.compute_dtype)
                return K.patch_embed_dgrad(dtok.contiguous(), w, C, H, self.patch_size)
        finally:
            for m, t in flags:
                m.training = t

    def forward_features(self, x):
        """[B,C,H,W] -> tokens [B,N,d] after the transformer blocks (reference vit.py:235-271)."""
        require_device(x)
        if x.requires_grad and torch.is_grad_enabled():
            # vitpe::patch_embed returns no gradient for `images` (the reference never differentiates them); autograd
            # would drop it without a word
            raise NotImplementedError("vitpe VisionTransformer: no gradient w.r.t. the `images` argument of "
                                      "vitpe::patch_embed (pass images that do not require grad)")
        B, C, H, W = x.shape
        return self._blocks(self._embed(x), (H // self.patch_size) * (W // self.patch_size))

    # the three stages of forward, shared with saliency (which differentiates from the tokens on)
    def _embed(self, x):
        """images -> tokens [B,N,d] (reference vit.py:245-258)"""
        ape = self.pos_embed.pos_embed if self.use_pos_embed_in_forward else None
        return torch.ops.vitpe.patch_embed(x, self.patch_embed.weight, self.patch_embed.bias, self.cls_token, ape,
                                           self.patch_size, self.compute_dtype == torch.bfloat16)[0]

    def _blocks(self, x, num_patches):
        """tokens -> tokens after the transformer blocks (reference vit.py:260-271)"""
        freqs_cis = None
        if self.use_rope:
            freqs_cis = (num_patches,)  # marker: the fused kernel builds (cos, sin) on the device itself
        for blk in self.blocks:
            x = blk(x, freqs_cis=freqs_cis)
        return x

    def _head(self, x):
        """logits [B,num_classes] fp32 (reference vit.py:273-285); the final LayerNorm is only evaluated on the class row,
        which is all the head reads."""
        return torch.ops.vitpe.head(x, self.norm.weight, self.norm.bias, self.head.weight, self.head.bias,
                                    self.norm.eps)[0]

    def attention_maps(self, x, layers=None, cls_only=False):
        """{layer: attention probabilities} of the eval forward of images x [B,C,H,W]: fp32 [B, H, N, N] per requested layer
        (default: every block), or [B, H, N] -- the class token's row -- with cls_only.  4 B H N^2 bytes a layer.

        Runs forward_features' own sequence under torch.no_grad() with eval semantics (no dropout, no stochastic depth, no
        RNG drawn; the training flags are restored afterwards): the tokens entering block l + 1 are the ordinary eval
        forward's, the probabilities of block l come from Block.attention_probs on its input."""
        require_device(x)
        want = self._want_layers("attention_maps", layers)
        with self._eval_no_grad():
            return {l: blk.attention_probs(t, freqs_cis=freqs_cis, cls_only=cls_only)
                    for l, blk, t, freqs_cis in self._block_inputs(x, want[-1] if want else -1) if l in want}

    # the analysis methods (attention_maps, attention_stats, attention_rollout) share the next three
    def _want_layers(self, what, layers):
        depth = len(self.blocks)
        want = list(range(depth)) if layers is None else sorted({int(l) for l in layers})
        if want and not (0 <= want[0] and want[-1] < depth):
            raise ValueError(f"vitpe {what}: layers must be in [0, {depth}), got {list(layers)}")
        return want

    @contextlib.contextmanager
    def _eval_no_grad(self):
        """eval semantics under torch.no_grad(); the training flags are restored afterwards, also on an exception"""
        flags = [(m, m.training) for m in self.modules()]
        self.eval()
        try:
            with torch.no_grad():
                yield
        finally:
            for m, was in flags:
                m.training = was

    def _block_inputs(self, x, last):
        """(l, block l, the tokens entering it, freqs_cis) for l = 0 .. last: forward_features' own sequence"""
        B, C, H, W = x.shape
        t = self._embed(x)
        freqs_cis = ((H // self.patch_size) * (W // self.patch_size),) if self.use_rope else None
        for l, blk in enumerate(self.blocks[:last + 1]):
            yield l, blk, t, freqs_cis
            if l < last:
                t = blk(t, freqs_cis=freqs_cis)

    def attention_stats(self, images, layers=None):
        """{layer: fp32 [B, H, 4]} of the eval forward of images [B,C,H,W], for the requested layers (default: every block):
        per head the mean attention distance in pixels (kernels.STAT_DISTANCE; patch queries and keys, unit = patch_size),
        the mean row entropy in nats (STAT_ENTROPY), the mean attention of the patch queries on the class token
        (STAT_CLS_MASS) and the entropy of the class row (STAT_CLS_ENTROPY) -- the numbers usually reduced from
        attention_maps, computed inside the kernel (Block.attention_stats): 16 bytes per (image, head), no [N, N] map is
        stored.  The contract of attention_maps: eval semantics under torch.no_grad(), no RNG drawn, training flags
        restored, the tokens entering block l + 1 are the ordinary eval forward's."""
        require_device(images)
        want = self._want_layers("attention_stats", layers)
        with self._eval_no_grad():
            return {l: blk.attention_stats(t, freqs_cis=freqs_cis, unit=float(self.patch_size))[0]
                    for l, blk, t, freqs_cis in self._block_inputs(images, want[-1] if want else -1) if l in want}

    def attention_rollout(self, images, start_layer=0, residual=0.5):
        """Attention rollout (Abnar & Zuidema) of the eval forward of images [B,C,H,W] -> fp32 [B, N]: the class token's row
        of A^_{L-1} ... A^_{start_layer}, A^_l = (1 - residual) mean_h A_{l,h} + residual I.  Rows of A^ sum to 1, so does
        the result; [:, 1:] viewed as grid x grid is the rollout map.

        One eval forward keeps every block's input (L B N d elements); then, from the top block down, the row vector
        v (e_cls to start with) is multiplied into the block's maps inside the statistics kernel (Block.attention_stats with
        weights=v: colsum = v . A_h per head) and mixed, v <- (1 - residual) mean_h colsum + residual v.  No [N, N] tensor
        exists at any point.  The contract of attention_maps otherwise."""
        require_device(images)
        depth = len(self.blocks)
        if not 0 <= int(start_layer) < depth:
            raise ValueError(f"vitpe attention_rollout: start_layer must be in [0, {depth}), got {start_layer}")
        if not 0.0 <= float(residual) <= 1.0:
            raise ValueError(f"vitpe attention_rollout: residual must be in [0, 1], got {residual}")
        with self._eval_no_grad():
            inputs = [(blk, t, freqs_cis) for _, blk, t, freqs_cis in self._block_inputs(images, depth - 1)]
            B, N = inputs[0][1].shape[:2]
            v = torch.zeros(B, N, dtype=torch.float32, device=images.device)
            v[:, 0] = 1.0
            for blk, t, freqs_cis in reversed(inputs[int(start_layer):]):
                colsum = blk.attention_stats(t, freqs_cis=freqs_cis, weights=v)[1]
                v = (1.0 - residual) * colsum.mean(dim=1) + residual * v
            return v

    def attention_relevance(self, images, target=None, start_layer=0, clamp=True):
        """Gradient-weighted attention relevance (Chefer, Gur & Wolf, "Generic Attention-model Explainability", ICCV 2021) of
        the eval forward of images [B,C,H,W] for the class target_b of each image -> fp32 [B, N]: the class token's row of
        R = (I + A~_{L-1}) ... (I + A~_{start_layer}),  A~_l = mean_h f(G_{l,h} . A_{l,h}),  with A the attention
        probabilities, G = d logits[b, target_b] / dA (the value rows held fixed: what a backward hook on the softmax sees)
        and f = max(0, .) under clamp (Chefer's rule), the signed product without.  target: LongTensor [B], or None = the
        arg-max class of each image.  [:, 1:] viewed as grid x grid is the relevance map; [:, 0] is returned as it is: the
        identity's 1 plus the class token's own relevance.

        One eval pass from the embedded tokens under enable_grad -- Block.forward's eval sequence, op for op -- keeps each
        block's norm1 output and its x + attn(norm1(x)); torch.autograd.grad w.r.t. the latter gives the gradient of every
        attention branch in one backward.  Then, from the top block down, the row vector v (e_cls to start with) goes
        through the relevance kernel (Attention.attention_relevance with weights=v) and v <- v + mean_h colsum.  No [N, N]
        tensor exists at any point.  saliency's contract: eval semantics (no dropout, no stochastic depth, no RNG drawn;
        the training flags are restored afterwards, also on an exception), no parameter's .grad is created or changed,
        `images` is left as it is, the result carries no graph."""
        depth = len(self.blocks)
        if not 0 <= int(start_layer) < depth:
            raise ValueError(f"vitpe attention_relevance: start_layer must be in [0, {depth}), got {start_layer}")
        if target is not None and (not torch.is_tensor(target) or target.dtype != torch.int64
                                   or tuple(target.shape) != (images.shape[0],)):
            raise ValueError("vitpe attention_relevance: target must be a LongTensor [B]")
        require_device(images)
        flags = [(m, m.training) for m in self.modules()]
        self.eval()
        try:
            logits, kept, freqs_cis = self._relevance_pass(images)
            with torch.enable_grad():
                if target is None:
                    target = logits.detach().argmax(dim=1)
                picked = logits.gather(1, target.to(logits.device).view(-1, 1)).sum()
                kept = kept[int(start_layer):]
                dmids = torch.autograd.grad(picked, inputs=[x_mid for _, _, x_mid in kept])
            with torch.no_grad():
                B, N = kept[0][1].shape[:2]
                v = torch.zeros(B, N, dtype=torch.float32, device=images.device)
                v[:, 0] = 1.0
                for (blk, n1, _), dmid in zip(reversed(kept), reversed(dmids)):
                    v = v + blk.attn.attention_relevance(n1, dmid, freqs_cis=freqs_cis, weights=v, clamp=clamp).mean(dim=1)
                return v
        finally:
            for m, was in flags:
                m.training = was

    def _relevance_pass(self, images):
        """(logits with their graph, [(block, norm1 output detached, x + attn(norm1 x))] bottom block first, freqs_cis):
        forward's own ops from the embedded tokens on, under enable_grad; the caller has set eval mode."""
        B, C, H, W = images.shape
        with torch.no_grad():
            tok = self._embed(images.detach())
        freqs_cis = ((H // self.patch_size) * (W // self.patch_size),) if self.use_rope else None
        kept = []
        with torch.enable_grad():
            x = tok.requires_grad_(True)
            for blk in self.blocks:   # Block.forward, eval branch
                n1 = torch.ops.vitpe.layer_norm(x, blk.norm1.weight, blk.norm1.bias, blk.norm1.eps)[0]
                x_mid = blk.attn(n1, freqs_cis=freqs_cis, resid=x)
                n2 = torch.ops.vitpe.layer_norm(x_mid, blk.norm2.weight, blk.norm2.bias, blk.norm2.eps)[0]
                x = blk.mlp(n2, resid=x_mid)
                kept.append((blk, n1.detach(), x_mid))
            return self._head(x), kept, freqs_cis

    def forward(self, x):
        """logits [B,num_classes] fp32 (reference vit.py:273-285); the final LayerNorm is only
        evaluated on the class row, which is all the head reads."""
        return self._head(self.forward_features(x))
