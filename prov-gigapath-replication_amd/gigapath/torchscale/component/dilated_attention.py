"""DilatedAttention for the MI355X path (reference: torchscale/component/dilated_attention.py).

Same constructor, parameter names (k_proj, v_proj, q_proj, out_proj, inner_attn_ln) and
forward signature as the reference module.  The forward runs the fused HIP pipeline:
one fused QKV GEMM, ONE gp_dilated_attn_fwd launch for every (segment, dilation) branch
(gather folded into the kernel's addressing, zero-pad keys analytic), gp_branch_merge_ln
(LSE merge + inner_attn_ln), and the out_proj GEMM.

Under autograd (an input that requires grad, or .train() with a parameter that does) the forward takes the
differentiable path instead: the projections and inner_attn_ln in torch from the live parameters, and the
attention core -- every branch and the merge -- through runtime.dilated_attention_grad, whose backward is one
gp_dilated_attn_bwd call (for a packed stream of several slides, runtime.dilated_attention_grad_varlen and one
gp_dilated_attn_bwd_varlen call).  Dropout is not implemented; every other case is the inference path, unchanged.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import runtime


class DilatedAttention(nn.Module):
    def __init__(self, args, embed_dim, num_heads, dropout=0.0, self_attention=False,
                 encoder_decoder_attention=False, subln=False):
        super().__init__()
        if not self_attention or encoder_decoder_attention:
            raise NotImplementedError("the slide encoder uses self-attention only")
        if not subln:
            raise NotImplementedError("the slide encoder uses subln (inner_attn_ln)")
        self.args = args
        self.embed_dim = embed_dim
        self.num_heads = num_heads
        self.head_dim = embed_dim // num_heads
        self.scaling = self.head_dim ** -0.5
        self.dropout = dropout
        self.self_attention = True
        # registration order = reference state-dict order (multihead_attention.py:43-53)
        self.k_proj = nn.Linear(embed_dim, embed_dim, bias=True)
        self.v_proj = nn.Linear(embed_dim, embed_dim, bias=True)
        self.q_proj = nn.Linear(embed_dim, embed_dim, bias=True)
        self.out_proj = nn.Linear(embed_dim, embed_dim, bias=True)
        self.inner_attn_ln = nn.LayerNorm(embed_dim, eps=args.layernorm_eps)
        self._packed = None
        self._packed_sig = None
        self._scratch = None

    def packed(self, dev, act: torch.dtype = torch.bfloat16) -> runtime.PackedAttention:
        sig = (str(dev), runtime.param_signature(self), act)
        if sig != self._packed_sig:
            self._packed = runtime.PackedAttention.from_module(self, dev, act)
            self._packed_sig = sig
        return self._packed

    def _differentiable(self, query, key, value) -> bool:
        if not torch.is_grad_enabled():
            return False
        if query.requires_grad or key.requires_grad or value.requires_grad:
            return True
        return self.training and any(p.requires_grad for p in self.parameters())

    def _forward_grad(self, query, key, value, slide_lens=None):
        """The differentiable path: torch projections / LayerNorm around the native core.  The Q scale
        D^-0.5 log2 e is folded into the Q weight and bias in fp32 before their cast, as PackedAttention does.
        slide_lens: the input is [1, T, E], slides of those lengths packed token-major; the core is then
        runtime.dilated_attention_grad_varlen (every slide its own segment schedule, D = 48)."""
        B, L, E = query.shape
        H, D = self.num_heads, self.head_dim
        if slide_lens is not None and (B != 1 or L != sum(slide_lens)):
            raise ValueError("DilatedAttention: a packed input must be [1, sum(slide_lens), E], got %s"
                             % (tuple(query.shape),))
        act = runtime.act_dtype()
        prescaled = D in (48, 64)
        qs = (D ** -0.5) * runtime.LOG2E if prescaled else 1.0
        M = B * L

        def wb(lin, scale=1.0):
            return lin.weight.float() * scale, lin.bias.float() * scale

        (wq, bq), (wk, bk), (wv, bv) = wb(self.q_proj, qs), wb(self.k_proj), wb(self.v_proj)
        if key is query and value is query:
            qkv = F.linear(query.reshape(M, E).to(act), torch.cat([wq, wk, wv], 0).to(act),
                           torch.cat([bq, bk, bv], 0).to(act))
        else:
            qkv = torch.cat([F.linear(t.reshape(M, E).to(act), w.to(act), b.to(act))
                             for t, w, b in ((query, wq, bq), (key, wk, bk), (value, wv, bv))], 1)
        if slide_lens is not None:
            merged = runtime.dilated_attention_grad_varlen(qkv, slide_lens, H, D, self.args.segment_length,
                                                           self.args.dilated_ratio)
        else:
            merged = runtime.dilated_attention_grad(qkv, B, L, H, D, self.args.segment_length,
                                                    self.args.dilated_ratio, prescaled)
        ln = self.inner_attn_ln
        if runtime.rows_fusable(E):
            a = runtime.layernorm_act_grad(merged, ln)        # one kernel each way, merged the only tensor saved
        else:
            a = F.layer_norm(merged.float(), (E,), ln.weight.float(), ln.bias.float(), ln.eps).to(act)
        out = F.linear(a, self.out_proj.weight.to(act), self.out_proj.bias.to(act))
        return out.view(B, L, E).to(query.dtype), None

    @runtime.compute_format
    def forward(self, query, key, value, incremental_state=None, key_padding_mask=None, attn_mask=None,
                rel_pos=None, is_first_step=False, is_causal=False):
        if incremental_state is not None or is_causal or rel_pos is not None or attn_mask is not None:
            raise NotImplementedError("incremental/causal/rel_pos/attn_mask are not on the slide-encoder path")
        if self.training and self.dropout > 0:
            raise RuntimeError("DilatedAttention (MI355X path) has no dropout: call .eval() or set dropout=0")
        B, L, E = query.shape
        if E != self.embed_dim or key.shape != query.shape or value.shape != query.shape:
            raise ValueError("query/key/value must all be [B, L, %d]" % self.embed_dim)
        dev = query.device
        if dev.type != "cuda":
            raise RuntimeError("DilatedAttention (MI355X path) needs ROCm device tensors")
        if self._differentiable(query, key, value):
            return self._forward_grad(query, key, value)
        act = runtime.act_dtype()
        pa = self.packed(dev, act)
        M = B * L
        qkv = torch.empty(M, 3 * E, dtype=act, device=dev)
        if key is query and value is query:
            torch.addmm(pa.b_qkv, query.reshape(M, E).to(act), pa.w_qkv.t(), out=qkv)
        else:
            for i, t in enumerate((query, key, value)):
                torch.addmm(pa.b_qkv[i * E:(i + 1) * E], t.reshape(M, E).to(act),
                            pa.w_qkv[i * E:(i + 1) * E].t(), out=qkv[:, i * E:(i + 1) * E])
        key_ = (B, L, pa.H, pa.D, tuple(pa.segs), tuple(pa.ratios), act)
        if self._scratch is None or self._scratch.key != key_:
            self._scratch = runtime.AttentionScratch(dev, B, L, pa.H, pa.D, pa.segs, pa.ratios, act)
        merged = torch.empty(M, E, dtype=act, device=dev)
        runtime.dilated_attention_core(pa, qkv, B, L, self._scratch, merged)
        out = torch.addmm(pa.b_o_act, merged, pa.w_o.t())
        return out.view(B, L, E).to(query.dtype), None
