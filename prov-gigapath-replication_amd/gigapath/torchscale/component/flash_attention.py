"""Operator seam of the reference: ``flash_attn_func`` (torchscale/component/flash_attention.py:13-16).

On the reference this binds flash-attn 2.5.8 (CUDA) or xformers; here it binds the gfx950
MFMA kernel behind ``gp_seg_attn_fwd`` (bf16) / ``gp_seg_attn_fwd_f16`` (fp16).  Same contract:
q, k, v [B, L, H, D], non-causal, no mask, dropout 0; returns (out [B, L, H, D] in q's dtype,
softmax_lse [B, H, L] fp32, natural log).  fp16 inputs (the reference pipeline's autocast,
pipeline.py:186-187) compute in fp16 as flash-attn does; bf16 in bf16; fp32 inputs (which flash-attn
rejects) are computed in bf16.

When grad mode is on and an input requires grad, the call goes through an autograd Function whose
backward is ``gp_seg_attn_bwd`` (what flash-attn's CUDA backward is on the reference); the LSE is marked
non-differentiable, as the reference uses it (dilated_attention.py:119-124, under torch.no_grad()).
Otherwise nothing is saved and no extra launch is made.
"""
from __future__ import annotations

import torch

from ... import _hip


def _forward(qb, kb, vb, softmax_scale):
    B, L, H, D = qb.shape
    out = torch.empty_like(qb)
    lse = torch.empty(B, H, L, dtype=torch.float32, device=qb.device)
    _hip.seg_attn_fwd(qb, kb, vb, out, lse, softmax_scale or 0.0)
    return out, lse


class _SegAttn(torch.autograd.Function):
    """q, k, v: contiguous, one 16-bit dtype (the casts stay outside, so autograd carries the gradients
    back through them)."""

    @staticmethod
    def forward(ctx, qb, kb, vb, softmax_scale):
        out, lse = _forward(qb, kb, vb, softmax_scale)
        ctx.save_for_backward(qb, kb, vb, out, lse)
        ctx.softmax_scale = softmax_scale or 0.0
        ctx.mark_non_differentiable(lse)
        return out, lse

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout, _dlse):
        qb, kb, vb, out, lse = ctx.saved_tensors
        dout = dout.to(qb.dtype).contiguous()
        dq, dk, dv = torch.empty_like(qb), torch.empty_like(kb), torch.empty_like(vb)
        _hip.seg_attn_bwd(qb, kb, vb, out, lse, dout, dq, dk, dv, ctx.softmax_scale)
        return dq, dk, dv, None


def flash_attn_func(q, k, v, dropout=0.0, bias=None, softmax_scale=None, is_causal=False):
    if bias is not None or is_causal or dropout != 0.0:
        raise NotImplementedError("gp_seg_attn_fwd: bias / causal / dropout are not on the slide-encoder path")
    if q.device.type != "cuda":
        raise RuntimeError("flash_attn_func (MI355X path) needs ROCm device tensors")
    B, L, H, D = q.shape
    dt = torch.float16 if q.dtype == torch.float16 else torch.bfloat16
    qb, kb, vb = (t.to(dt).contiguous() for t in (q, k, v))
    if torch.is_grad_enabled() and (q.requires_grad or k.requires_grad or v.requires_grad):
        out, lse = _SegAttn.apply(qb, kb, vb, softmax_scale)
    else:
        out, lse = _forward(qb, kb, vb, softmax_scale)
    return out.to(q.dtype), lse
