"""LongNet encoder stack (reference: torchscale/architecture/encoder.py:25-399), subln.

Module tree and parameter names match the reference (layers.{i}.self_attn.*,
self_attn_layer_norm, ffn.{fc1,fc2,ffn_layernorm}, final_layer_norm, layer_norm) so
reference state dicts load unchanged.  ``Encoder.forward`` keeps the reference's signature
and return dict; the arithmetic runs through runtime.EncoderEngine (HIP kernels + hipBLASLt).
LongNetViT bypasses it to fuse the embedding with the first LayerNorm.

EncoderLayer and Encoder are trainable on opt-in (`trainable`, set by LongNetViT.enable_training): with autograd
live they take an eager differentiable path -- an fp32 residual stream around DilatedAttention's and
FeedForwardNetwork's differentiable paths, with dropout and drop-path as in the reference (encoder.py:116-162).  The
LayerNorms, the output dropouts, drop-path and the residual adds run as the training row kernels
(runtime.layernorm_act_grad / resid_drop_ln_grad / resid_drop_grad) at the widths they cover, and as
torch ops in fp32 otherwise or with GIGAPATH_TRAIN_ROWS_FUSED=0.  Every other call is the inference path, unchanged.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import _hip, runtime
from ..component.dilated_attention import DilatedAttention
from ..component.feedforward_network import FeedForwardNetwork


def _ln_to_act(x32: torch.Tensor, ln: nn.LayerNorm, out_act: torch.Tensor):
    """out = LayerNorm(x) for an fp32 [M, E] residual stream, rounded to the 16-bit activation format
    (standalone-module entry only)."""
    dev = x32.device
    tmp = torch.empty_like(x32)
    _hip.layernorm_f32(x32, x32.shape[1], runtime._f32(ln.weight, dev), runtime._f32(ln.bias, dev), float(ln.eps),
                       tmp, x32.shape[0], x32.shape[1])
    out_act.copy_(tmp)


def _ln_grad(x32: torch.Tensor, ln: nn.LayerNorm) -> torch.Tensor:
    """LayerNorm of the fp32 residual stream in fp32 (differentiable path)."""
    return F.layer_norm(x32, (x32.shape[-1],), ln.weight.float(), ln.bias.float(), ln.eps)


def run_layers_grad(layers, x, on_state=None, slide_lens=None):
    """The chain of the layers' differentiable forwards on the fp32 residual stream x [B, L, E].  Each layer is
    handed the next layer's self_attn_layer_norm, so that layer i's last residual add and layer i + 1's first
    LayerNorm are one call (EncoderLayer._forward_grad); the per-layer states are the r outputs, the same bits as
    calling the layers one by one.  With slide_lens, x is [1, T, E]: the slides of those lengths packed token-major
    (T = sum(slide_lens)); every row op runs over the T rows, the attention core is the varlen one and drop-path
    draws once per slide."""
    if slide_lens is not None and (x.dim() != 3 or x.shape[0] != 1 or x.shape[1] != sum(slide_lens)):
        raise ValueError("run_layers_grad: a packed stream must be [1, sum(slide_lens), E], got %s" % (tuple(x.shape),))
    a = None
    n = len(layers)
    for i, layer in enumerate(layers):
        if not runtime.rows_fusable(layer.embed_dim, layer.dropout if layer.training else 0.0):
            x, a = layer._forward_grad(x, slide_lens=slide_lens), None   # the torch composition, layer by layer
        elif i + 1 < n:
            x, a = layer._forward_grad(x, a, layers[i + 1].self_attn_layer_norm, slide_lens=slide_lens)
            a = a.reshape(-1, a.shape[-1])
        else:
            x = layer._forward_grad(x, a, slide_lens=slide_lens)
        if on_state is not None:
            on_state(x)
    return x


class EncoderLayer(nn.Module):
    trainable = False       # opt-in to the differentiable path (LongNetViT.enable_training)

    def __init__(self, args, depth, is_moe_layer=False, is_encoder_decoder=False):
        super().__init__()
        if is_moe_layer or is_encoder_decoder:
            raise NotImplementedError("MoE / encoder-decoder layers are outside the slide-encoder path")
        self.args = args
        self.embed_dim = args.encoder_embed_dim
        self.self_attn = self.build_self_attention(self.embed_dim, args)
        self.self_attn_layer_norm = nn.LayerNorm(self.embed_dim, eps=args.layernorm_eps)
        self.dropout = args.dropout
        self.drop_path_prob = (float(np.linspace(0, args.drop_path_rate, args.encoder_layers)[depth])
                               if args.drop_path_rate > 0 else 0.0)
        self.ffn_dim = args.encoder_ffn_embed_dim
        self.ffn = FeedForwardNetwork(self.embed_dim, self.ffn_dim, args.activation_fn, args.dropout,
                                      args.activation_dropout, args.layernorm_eps, args.subln)
        self.final_layer_norm = nn.LayerNorm(self.embed_dim, eps=args.layernorm_eps)

    def build_self_attention(self, embed_dim, args):
        return DilatedAttention(args, embed_dim, args.encoder_attention_heads, dropout=args.attention_dropout,
                                self_attention=True, subln=args.subln)

    def _forward_grad(self, x, a_in=None, next_ln=None, slide_lens=None):
        """The differentiable path (reference encoder.py:116-162, pre-LN, alpha = 1) on an fp32 residual
        stream: LN -> self_attn -> dropout -> drop-path -> residual -> LN -> FFN -> drop-path -> residual.

        At the widths the training row kernels cover (runtime.rows_fusable) the rows are three fused calls:
        LN1 (runtime.layernorm_act_grad), attention-output dropout + drop-path + residual + LN2
        (runtime.resid_drop_ln_grad), FFN-output dropout + drop-path + residual (runtime.resid_drop_grad).
        A stack (run_layers_grad) hands over a_in, this layer's LN1 output computed by the previous layer's last
        call, and next_ln, the next layer's self_attn_layer_norm: the return value is then (r, next_ln(r) in the
        16-bit format), the same bits as the two calls apart.  Both are ignored by the torch composition.

        slide_lens: x is a packed [1, T, E] stream of slides of those lengths (run_layers_grad): the attention
        core is the varlen one and drop-path draws one factor per slide, in slide order, for the slide's rows."""
        if self.training and self.self_attn.dropout > 0:
            raise RuntimeError("EncoderLayer (MI355X path): attention dropout is not implemented in training; "
                               "set attention_dropout=0")
        act = runtime.act_dtype()
        res = x.float()
        if runtime.rows_fusable(self.embed_dim, self.dropout if self.training else 0.0):
            return self._forward_grad_fused(res, act, a_in, next_ln, slide_lens)
        a = _ln_grad(res, self.self_attn_layer_norm).to(act)
        a, _ = self._attn_grad(a, slide_lens)
        a = F.dropout(a.float(), self.dropout, self.training)
        res = res + runtime.drop_path(a, self.drop_path_prob, self.training, slide_lens)
        f = self.ffn._forward_grad(_ln_grad(res, self.final_layer_norm).to(act))
        return res + runtime.drop_path(f.float(), self.drop_path_prob, self.training, slide_lens)

    def _attn_grad(self, a, slide_lens):
        """self_attn on the differentiable path: the module call, or for a packed stream its _forward_grad with the
        slide lengths."""
        if slide_lens is None:
            return self.self_attn(a, a, a)
        return self.self_attn._forward_grad(a, a, a, slide_lens=slide_lens)

    def _forward_grad_fused(self, res, act, a_in, next_ln, slide_lens=None):
        B, L, E = res.shape
        M = B * L
        dev = res.device
        x2 = res.reshape(M, E)
        a = a_in if a_in is not None else runtime.layernorm_act_grad(x2, self.self_attn_layer_norm)
        a = a.view(B, L, E)
        y, _ = self._attn_grad(a, slide_lens)
        s = runtime.drop_path_scale(B, self.drop_path_prob, self.training, dev, slide_lens)
        r, a2 = runtime.resid_drop_ln_grad(x2, y.reshape(M, E).to(act), self.final_layer_norm, self.dropout, s,
                                           self.training)
        f = self.ffn._forward_grad_core(a2)
        s = runtime.drop_path_scale(B, self.drop_path_prob, self.training, dev, slide_lens)
        if next_ln is None:
            return runtime.resid_drop_grad(r, f, self.dropout, s, self.training).view(B, L, E)
        r2, a_next = runtime.resid_drop_ln_grad(r, f, next_ln, self.dropout, s, self.training)
        return r2.view(B, L, E), a_next

    @runtime.compute_format
    def forward(self, x, encoder_padding_mask=None, attn_mask=None, rel_pos=None, multiway_split_position=None,
                incremental_state=None, slide_lens=None):
        if runtime.takes_grad_path(self, x):
            if x.device.type != "cuda":
                raise RuntimeError("EncoderLayer (MI355X path) needs ROCm device tensors")
            return self._forward_grad(x, slide_lens=slide_lens).to(x.dtype), None
        if slide_lens is not None:
            raise RuntimeError("EncoderLayer (MI355X path): slide_lens is a training-path argument; inference packs "
                               "slides through LongNetViT.forward_packed")
        if self.training and (self.dropout > 0 or self.drop_path_prob > 0):
            raise RuntimeError("EncoderLayer (MI355X path) is inference-only: call .eval()")
        B, L, E = x.shape
        dev = x.device
        if dev.type != "cuda":
            raise RuntimeError("EncoderLayer (MI355X path) needs ROCm device tensors")
        eng = runtime.EncoderEngine()
        act = runtime.act_dtype()
        pl = runtime.PackedLayer.from_module(self, dev, act)
        eng.layers = [pl]
        ws = runtime.Workspace(dev, B, L, E, self.ffn_dim, pl.attn.H, pl.attn.segs, pl.attn.ratios, act)
        ws.x.copy_(x.reshape(B * L, E))
        _ln_to_act(ws.x, self.self_attn_layer_norm, ws.a)
        eng.run_layers(ws, B, L)
        return ws.x.view(B, L, E).to(x.dtype), None


class Encoder(nn.Module):
    trainable = False       # opt-in to the differentiable path (LongNetViT.enable_training)

    def __init__(self, args, embed_tokens=None, embed_positions=None, output_projection=None,
                 is_encoder_decoder=False, **kwargs):
        super().__init__(**kwargs)
        if embed_tokens is not None or embed_positions is not None or output_projection is not None:
            raise NotImplementedError("token/position embeddings and output projections are not used by LongNetViT")
        self.args = args
        self.layers = nn.ModuleList([self.build_encoder_layer(args, depth=i) for i in range(args.encoder_layers)])
        self.num_layers = len(self.layers)
        self.layer_norm = (nn.LayerNorm(args.encoder_embed_dim, eps=args.layernorm_eps)
                           if args.encoder_normalize_before and args.normalize_output else None)
        self.engine = runtime.EncoderEngine()

    def build_encoder_layer(self, args, depth, is_moe_layer=False, is_encoder_decoder=False):
        return EncoderLayer(args, depth, is_moe_layer=is_moe_layer, is_encoder_decoder=is_encoder_decoder)

    def check_eval(self):
        if self.training and (self.args.dropout > 0 or self.args.drop_path_rate > 0):
            raise RuntimeError("the MI355X slide encoder is inference-only: call model.eval()")

    @runtime.compute_format
    def forward(self, src_tokens, encoder_padding_mask=None, attn_mask=None, return_all_hiddens=False,
                token_embeddings=None, multiway_split_position=None, features_only=False,
                incremental_state=None, positions=None, **kwargs):
        if token_embeddings is None:
            raise NotImplementedError("LongNetViT feeds token_embeddings; src_tokens lookup is not on the path")
        if attn_mask is not None or incremental_state is not None:
            raise NotImplementedError("attn_mask / incremental_state are not on the slide-encoder path")
        grad_path = runtime.takes_grad_path(self, token_embeddings)
        if not grad_path:
            self.check_eval()
        x_in = token_embeddings
        B, L, E = x_in.shape
        dev = x_in.device
        if dev.type != "cuda":
            raise RuntimeError("Encoder (MI355X path) needs ROCm device tensors")
        if encoder_padding_mask is None:
            encoder_padding_mask = torch.zeros(B, L, dtype=torch.bool, device=dev)
        else:
            # encoder.py:358: masked embeddings are zeroed before the first layer (and in
            # encoder_states[0]); the flash attention path does not see the mask
            # (multihead_attention.py:103), so padded tokens stay keys of every branch
            if encoder_padding_mask.shape != (B, L):
                raise ValueError("encoder_padding_mask must be [B, L] = [%d, %d], got %s"
                                 % (B, L, tuple(encoder_padding_mask.shape)))
            x_in = x_in * (1 - encoder_padding_mask.to(dev).unsqueeze(-1).type_as(x_in))
        if grad_path:
            # eager, layer by layer, on an fp32 residual stream (EncoderLayer._forward_grad)
            x = x_in.float()
            states = [x_in] if return_all_hiddens else []
            x = run_layers_grad(self.layers, x, (lambda r: states.append(r.to(x_in.dtype)))
                                if return_all_hiddens else None)
            if self.layer_norm is not None:
                x = _ln_grad(x, self.layer_norm)
            return {"encoder_out": x.to(x_in.dtype), "encoder_embedding": token_embeddings,
                    "encoder_padding_mask": encoder_padding_mask, "encoder_states": states,
                    "l_aux": [None] * self.num_layers}
        layers = self.engine.pack(self, dev)
        pa = layers[0].attn
        ws = self.engine.workspace(dev, B, L, E, self.args.encoder_ffn_embed_dim, pa.H, pa.segs, pa.ratios)
        ws.x.copy_(x_in.reshape(B * L, E))
        _ln_to_act(ws.x, self.layers[0].self_attn_layer_norm, ws.a)
        states = [x_in] if return_all_hiddens else []

        def hook(i):
            if return_all_hiddens:
                states.append(ws.x.view(B, L, E).to(x_in.dtype, copy=True))

        self.engine.run_layers(ws, B, L, hook)
        x = ws.x
        if self.layer_norm is not None:
            out = torch.empty_like(x)
            _hip.layernorm_f32(x, E, runtime._f32(self.layer_norm.weight, dev), runtime._f32(self.layer_norm.bias, dev),
                               float(self.layer_norm.eps), out, B * L, E)
            x = out
        return {"encoder_out": x.view(B, L, E).to(x_in.dtype), "encoder_embedding": token_embeddings,
                "encoder_padding_mask": encoder_padding_mask, "encoder_states": states, "l_aux": [None] * self.num_layers}
