"""FFN of the LongNet encoder layer (reference: torchscale/component/feedforward_network.py:105-142).

fc1 -> exact-erf GELU in fp32 -> ffn_layernorm -> fc2.  fc1/fc2 run on hipBLASLt in bf16 (fp16 under
the caller's fp16 autocast);
GELU and the 3072-wide LayerNorm are one HIP kernel (gp_gelu_layernorm).

With `trainable` set (LongNetViT.enable_training) and autograd live -- an input that requires grad, or .train() with
a parameter that does -- the forward takes the differentiable path: fc1 / fc2 as F.linear from the live parameters,
the GELU + LayerNorm middle through runtime.gelu_layernorm_grad (one kernel each way, only the pre-activation
saved), then the output dropout.  Every other call is the inference path, unchanged.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import _hip, runtime


class FeedForwardNetwork(nn.Module):
    trainable = False       # opt-in to the differentiable path (LongNetViT.enable_training)

    def __init__(self, embed_dim, ffn_dim, activation_fn="gelu", dropout=0.0, activation_dropout=0.0,
                 layernorm_eps=1e-5, subln=True):
        super().__init__()
        if str(activation_fn) != "gelu" or not subln:
            raise NotImplementedError("the slide encoder FFN is gelu + subln")
        self.embed_dim = embed_dim
        self.dropout = dropout
        self.activation_dropout = activation_dropout
        self.fc1 = nn.Linear(embed_dim, ffn_dim)
        self.fc2 = nn.Linear(ffn_dim, embed_dim)
        self.ffn_layernorm = nn.LayerNorm(ffn_dim, eps=layernorm_eps)

    def _forward_grad_core(self, x):
        """The differentiable path before the output dropout, in the activation format (the encoder layer fuses
        that dropout into its residual add).  Reference feedforward_network.py:131-142: the fused middle when there is
        no activation dropout, GIGAPATH_TRAIN_FFN_FUSED is on and the width is one the kernel covers; otherwise
        the torch composition with the activation dropout between the GELU and ffn_layernorm."""
        shape = x.shape
        act = runtime.act_dtype()
        ln = self.ffn_layernorm
        h = F.linear(x.reshape(-1, shape[-1]).to(act), self.fc1.weight.to(act), self.fc1.bias.to(act))
        if self.activation_dropout == 0 and runtime.TRAIN_FFN_FUSED and h.shape[1] in runtime.GELU_LN_COLS:
            y = runtime.gelu_layernorm_grad(h, ln.weight, ln.bias, ln.eps)
        else:
            y = runtime.gelu_layernorm_torch(h, ln.weight, ln.bias, ln.eps, self.activation_dropout, self.training)
        return F.linear(y, self.fc2.weight.to(act), self.fc2.bias.to(act)).view(shape)

    def _forward_grad(self, x):
        """The differentiable path with the output dropout (standalone calls, and the layer's torch composition)."""
        return F.dropout(self._forward_grad_core(x), self.dropout, self.training).to(x.dtype)

    @runtime.compute_format
    def forward(self, x):
        if x.device.type != "cuda":
            raise RuntimeError("FeedForwardNetwork (MI355X path) needs ROCm device tensors")
        if runtime.takes_grad_path(self, x):
            return self._forward_grad(x)
        shape = x.shape
        dev = x.device
        act = runtime.act_dtype()
        h = torch.addmm(self.fc1.bias.to(dev, act), x.reshape(-1, shape[-1]).to(act), self.fc1.weight.to(dev, act).t())
        _hip.gelu_layernorm(h, runtime._f32(self.ffn_layernorm.weight, dev), runtime._f32(self.ffn_layernorm.bias, dev),
                            float(self.ffn_layernorm.eps), h, h.shape[0], h.shape[1])
        y = torch.addmm(self.fc2.bias.to(dev, act), h, self.fc2.weight.to(dev, act).t())
        return y.view(shape).to(x.dtype)
