"""MI355X execution engine of the LongNet slide-encoder forward.

Per layer the engine issues 8 kernels on torch's current HIP stream (M = B*L tokens):

    qkv  = LN1(x) . Wqkv^T + bqkv         gp_linear_ln (MFMA GEMM, LN1 folded; layer 0: gp_linear of
                                           the pos-embed kernel's LN1)              [M, 3E] bf16
    attn = gp_dilated_attn_fwd(qkv)        ONE launch, all dilation branches  sparse o / lse
    a    = LN_inner(merge(attn))           gp_branch_merge_ln                 [M, E] bf16
    x   += a . Wo^T + bo                   gp_linear_resid (fp32 residual stream updated in the epilogue,
                                           which also writes xb = gamma2 (x - s) and LN statistics)
    f    = gelu(LN2(x) . W1^T + b1), stats gp_ffn_fc1_gelu_ln (LN2 folded; GELU + LN statistics epilogue)
    x   += LN_ffn(f) . W2^T + b2           gp_ffn_fc2_ln_resid (LN folded; residual + the next layer's
                                           xb = gamma1' (x - s) and statistics in the epilogue)

(plus a split-K reduce after a GEMM whose last round of tiles is split).  That fused form (each LayerNorm
folded into the GEMM that consumes it, from the 16-bit xb = act(gamma (x - s)) and per-256-column
statistics its producer wrote; s = the row mean before the add; gp_gemm_impl.h) runs under
GIGAPATH_RESID_FUSED=1.  The default (round 6, faster: see RESID_FUSED below), and shapes outside the GEMM
kernels' instantiations, GIGAPATH_OWN_GEMMS=0 or GIGAPATH_FFN_FUSED=0, run the round-3 sequence:
gp_linear out-proj -> gp_residual_layernorm -> gp_ffn_fc1_gelu -> gp_ffn_fc2_ln -> gp_residual_layernorm
(hipBLASLt for uncovered GEMMs; for an uncovered FFN hipBLASLt fc1 + gp_gelu_layernorm + hipBLASLt fc2).

which is EncoderLayer.forward (torchscale/architecture/encoder.py:116-162) with
DilatedAttention.forward (component/dilated_attention.py:133-217) and the FFN
(component/feedforward_network.py:131-142) in eval mode.  The residual stream stays fp32;
GEMM operands are 16-bit (bf16, or fp16 under the caller's fp16 autocast) with fp32 accumulation.  Weights are packed once per parameter
version (fused QKV weight, bf16 GEMM operands, fp32 norms/biases) and workspaces are reused
across calls of the same shape.  No CPU fallback exists: every non-GEMM op is a HIP kernel.

When the caller reads only the CLS row of each slide (LongNetViT with global_pool off), the last layer runs its
QKV GEMM in full and the rest for those rows alone (cls_tail: gp_cls_attn_merge_ln, then the same entry points
at M = slides).  On the dense [B, L] forward the layer before it then runs, after its attention, for
the rows the CLS query's keys name (key_row_tail: gp_branch_merge_ln_rows, the same entry points at M = B |S|, the
last QKV GEMM on those rows and gp_cls_attn_merge_ln_map).
"""
from __future__ import annotations

import contextlib
import functools
import math
import os
import threading
from collections import OrderedDict
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _hip

_TUNED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tuned", "tunableop_results.csv")
_tuned_loaded = False


def use_tuned_gemms(dev=None):
    """Load the hipBLASLt solutions tools/tune_gemms.py selected for the slide encoder's GEMM
    shapes (PyTorch TunableOp, tuning itself off).  Shapes not in the file keep hipBLASLt's
    default heuristic.  GIGAPATH_NO_TUNED_GEMMS=1 disables it."""
    global _tuned_loaded
    path = os.environ.get("GIGAPATH_TUNED_GEMMS_FILE", _TUNED)     # an alternative tuning (A/B runs)
    if _tuned_loaded or os.environ.get("GIGAPATH_NO_TUNED_GEMMS") == "1" or not os.path.exists(path):
        return
    if dev is None or torch.device(dev).type != "cuda":
        return
    _tuned_loaded = True
    torch.cuda.tunable.enable(True)
    torch.cuda.tunable.tuning_enable(False)
    torch.cuda.tunable.record_untuned_enable(False)
    torch.cuda.tunable.read_file(path)


_ACT = threading.local()


def call_act_dtype(module: Optional[torch.nn.Module] = None) -> torch.dtype:
    """The 16-bit activation format of a call: fp16 inside torch.autocast("cuda", float16) -- the
    reference pipeline runs the slide encoder that way (pipeline.py:186-187), so its Linear layers
    and flash-attn compute in fp16 -- or for a module whose parameters are fp16 (model.half());
    bf16 (BASELINE's dtype) otherwise, including under bf16 autocast."""
    if torch.is_autocast_enabled("cuda"):
        return torch.float16 if torch.get_autocast_dtype("cuda") == torch.float16 else torch.bfloat16
    if module is not None:
        p = next(module.parameters(), None)
        if p is not None and p.dtype == torch.float16:
            return torch.float16
    return torch.bfloat16


def act_dtype() -> torch.dtype:
    """The activation format of the compute_format call in progress on this thread (bf16 outside)."""
    return getattr(_ACT, "dtype", None) or torch.bfloat16


def compute_format(fn):
    """Decorator of the module forwards: fixes the call's activation format (call_act_dtype) for the
    whole call, nested forwards included, then runs with autocast off (autocast must not retarget
    the GEMMs that write into the 16-bit workspaces with out=).  Every 16-bit activation, GEMM operand
    and kernel format of the call follows it; the residual stream, LN parameters, LSEs and readouts
    stay fp32; outputs keep the model's parameter dtype, as the reference's autocast LayerNorm
    readout does."""
    @functools.wraps(fn)
    def wrapped(self, *args, **kw):
        outer = getattr(_ACT, "dtype", None)
        _ACT.dtype = outer if outer is not None else call_act_dtype(self)
        try:
            with torch.autocast("cuda", enabled=False):
                return fn(self, *args, **kw)
        finally:
            _ACT.dtype = outer
    return wrapped


# ------------------------------------------------------------------------------------------
# optional live timing of the hot kernels (bench.py: roofline "achieved" numbers)
# ------------------------------------------------------------------------------------------
class KernelTimer:
    """Records HIP events (on the launch stream) around selected kernels when enabled."""

    def __init__(self):
        self.enabled = False
        self.events: Dict[str, List[Tuple[torch.cuda.Event, torch.cuda.Event]]] = {}

    def reset(self):
        self.events = {}

    def span(self, name: str):
        timer = self

        class _Span:
            def __enter__(self_inner):
                if timer.enabled:
                    self_inner.e0 = torch.cuda.Event(enable_timing=True)
                    self_inner.e1 = torch.cuda.Event(enable_timing=True)
                    self_inner.e0.record()
                return self_inner

            def __exit__(self_inner, *exc):
                if timer.enabled:
                    self_inner.e1.record()
                    timer.events.setdefault(name, []).append((self_inner.e0, self_inner.e1))
                return False

        return _Span()

    def totals_ms(self) -> Dict[str, Tuple[int, float]]:
        """name -> (launch count, summed milliseconds).  Synchronises."""
        torch.cuda.synchronize()
        return {k: (len(v), sum(a.elapsed_time(b) for a, b in v)) for k, v in self.events.items()}


TIMER = KernelTimer()


# ------------------------------------------------------------------------------------------
# geometry (dilated_attention.py:16-31, 76-98)
# ------------------------------------------------------------------------------------------
def branch_geometry(L: int, sl: int, r: int) -> Tuple[int, int, int]:
    """(s, nseg, m) of one branch at sequence length L."""
    s = min(sl, L)
    return s, -(-L // s), -(-s // r)


def attention_valid_flops(L: int, segs: Sequence[int], ratios: Sequence[int], H: int, D: int, B: int = 1) -> float:
    """Algorithmic FLOPs of one layer's dilated attention: 4*D*c^2 per (segment, head), c = real
    (non-pad) tokens the head sees in that segment.  Zero pads count 0."""
    tot = 0
    for sl, r in zip(segs, ratios):
        s, nseg, m = branch_geometry(L, sl, r)
        hp = H + ((r - H % r) % r)
        hpg = hp // r
        for n in range(nseg):
            rem = min(L - n * s, s)
            for h in range(H):
                j = h // hpg
                lim = rem - j
                c = -(-lim // r) if lim > 0 else 0
                tot += 4 * D * c * c
    return float(tot * B)


# ------------------------------------------------------------------------------------------
# packed weights
# ------------------------------------------------------------------------------------------
def _act(t: torch.Tensor, dev, act: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """A 16-bit GEMM operand copy (bf16 or fp16)."""
    return t.detach().to(device=dev, dtype=act).contiguous()


def _bf16(t: torch.Tensor, dev) -> torch.Tensor:
    return _act(t, dev, torch.bfloat16)


def _f32(t: torch.Tensor, dev) -> torch.Tensor:
    return t.detach().to(device=dev, dtype=torch.float32).contiguous()


LOG2E = 1.4426950408889634


@dataclass
class PackedAttention:
    """Packed DilatedAttention weights.  The softmax scale D^-0.5 and log2(e) are folded into the
    Q rows of the fused projection (in fp32, before the single 16-bit rounding of the GEMM output),
    so the attention kernel consumes log2-domain logits (gp_dilated_attn_fwd q_log2_prescaled).
    16-bit operands are in `act` (bf16, or fp16 for the caller's fp16 autocast)."""
    E: int
    H: int
    D: int
    segs: List[int]
    ratios: List[int]
    w_qkv: torch.Tensor      # [3E, E] act (q * scale*log2e | k | v rows)
    b_qkv: torch.Tensor      # [3E] act
    w_o: torch.Tensor        # [E, E] act
    b_o: torch.Tensor        # [E] fp32 (added in the residual kernel)
    b_o_act: torch.Tensor    # [E] act (standalone module forward)
    ln_w: torch.Tensor
    ln_b: torch.Tensor
    ln_eps: float

    prescaled: bool = True
    b_qkv_f32: Optional[torch.Tensor] = None   # [3E] fp32 (gp_linear's bias)
    # fp16 packing only: the engine's QKV GEMMs write the V third of qkv in bf16 and the attention reads it so
    # (GP_FMT_F16_VBF16): bf16 P.V at the bf16 kernel's speed instead of the exact fp16 running-max kernel
    # (DESIGN §3.3).  Every engine producer and consumer of qkv passes it; the standalone module does not.
    v_bf16: bool = False

    def qkv_parts(self, qkv: torch.Tensor):
        """(q, k, v) column views of a fused [M, 3E] qkv buffer this layer's engine wrote, each with the dtype
        its bytes hold: with v_bf16 the V third of an fp16 qkv is bf16, so v is viewed as bfloat16 (reading
        qkv[:, 2E:] as fp16 would silently misread it).  Readers of ws.qkv outside the engine's own entry
        points go through here (advice r05)."""
        E = self.E
        q, k, v = qkv[:, :E], qkv[:, E:2 * E], qkv[:, 2 * E:3 * E]
        if self.v_bf16 and qkv.dtype == torch.float16:
            v = v.view(torch.bfloat16)
        return q, k, v

    @staticmethod
    def from_module(m, dev, act: torch.dtype = torch.bfloat16) -> "PackedAttention":
        E, H = m.embed_dim, m.num_heads
        D = E // H
        qs = (D ** -0.5) * LOG2E if D in (48, 64) else 1.0   # D=96 uses the generic kernel
        wq = m.q_proj.weight.detach().to(device=dev, dtype=torch.float32) * qs
        bq = m.q_proj.bias.detach().to(device=dev, dtype=torch.float32) * qs
        b_qkv = torch.cat([bq, _f32(m.k_proj.bias, dev), _f32(m.v_proj.bias, dev)], 0)
        return PackedAttention(
            E=E, H=H, D=D, segs=list(m.args.segment_length), ratios=list(m.args.dilated_ratio),
            w_qkv=_act(torch.cat([wq, _f32(m.k_proj.weight, dev), _f32(m.v_proj.weight, dev)], 0), dev, act),
            b_qkv=_act(b_qkv, dev, act), b_qkv_f32=_act(b_qkv, dev, act).float().contiguous(),
            w_o=_act(m.out_proj.weight, dev, act), b_o=_f32(m.out_proj.bias, dev),
            b_o_act=_act(m.out_proj.bias, dev, act),
            ln_w=_f32(m.inner_attn_ln.weight, dev), ln_b=_f32(m.inner_attn_ln.bias, dev),
            ln_eps=float(m.inner_attn_ln.eps), prescaled=D in (48, 64),
            v_bf16=(act == torch.float16 and D == 48 and OWN_GEMMS and _hip.gemm_supported(3 * E, E)))


@dataclass
class PackedLayer:
    attn: PackedAttention
    ln1_w: torch.Tensor
    ln1_b: torch.Tensor
    ln1_eps: float
    ln2_w: torch.Tensor
    ln2_b: torch.Tensor
    ln2_eps: float
    w1: torch.Tensor         # [F, E] act
    b1: torch.Tensor         # [F] act
    fln_w: torch.Tensor      # [F] fp32
    fln_b: torch.Tensor
    fln_eps: float
    w2: torch.Tensor         # [E, F] act
    b2: torch.Tensor         # [E] fp32
    # the fused FFN (gp_ffn_fc1_gelu / gp_ffn_fc2_ln), None when its kernels do not cover the shape:
    b1_f32: Optional[torch.Tensor] = None   # [F] fp32
    w2g: Optional[torch.Tensor] = None      # [E, F] act: W2 * gamma_ffn (LN weight folded into fc2)
    c2: Optional[torch.Tensor] = None       # [E] fp32: row sums of w2g as rounded
    d2: Optional[torch.Tensor] = None       # [E] fp32: W2 . beta_ffn + b2
    # the residual stream inside the GEMMs (gp_linear_ln / gp_ffn_fc1_gelu_ln fold the pre-LNs):
    c_qkv: Optional[torch.Tensor] = None    # [3E] fp32: w_qkv . gamma1 (w_qkv as rounded)
    d_qkv: Optional[torch.Tensor] = None    # [3E] fp32: w_qkv . beta1 + b_qkv
    c1: Optional[torch.Tensor] = None       # [F] fp32: w1 . gamma2
    d1: Optional[torch.Tensor] = None       # [F] fp32: w1 . beta2 + b1

    @property
    def ffn_fused(self) -> bool:
        return self.w2g is not None

    @property
    def resid_fused(self) -> bool:
        return self.c1 is not None

    @staticmethod
    def from_module(layer, dev, act: torch.dtype = torch.bfloat16) -> "PackedLayer":
        ffn = layer.ffn
        pl = PackedLayer(
            attn=PackedAttention.from_module(layer.self_attn, dev, act),
            ln1_w=_f32(layer.self_attn_layer_norm.weight, dev), ln1_b=_f32(layer.self_attn_layer_norm.bias, dev),
            ln1_eps=float(layer.self_attn_layer_norm.eps),
            ln2_w=_f32(layer.final_layer_norm.weight, dev), ln2_b=_f32(layer.final_layer_norm.bias, dev),
            ln2_eps=float(layer.final_layer_norm.eps),
            w1=_act(ffn.fc1.weight, dev, act), b1=_act(ffn.fc1.bias, dev, act),
            fln_w=_f32(ffn.ffn_layernorm.weight, dev), fln_b=_f32(ffn.ffn_layernorm.bias, dev),
            fln_eps=float(ffn.ffn_layernorm.eps),
            w2=_act(ffn.fc2.weight, dev, act), b2=_f32(ffn.fc2.bias, dev))
        F, E = pl.w1.shape
        if ffn_fusable(E, F) or resid_fusable(E, F):
            # LN(h) . W2^T + b2 = rstd (h . (W2 gamma)^T - mean c) + d  (csrc/gp_gemm_impl.h, "LN fold")
            w2 = ffn.fc2.weight.detach().to(device=dev, dtype=torch.float64)
            g = ffn.ffn_layernorm.weight.detach().to(device=dev, dtype=torch.float64)
            be = ffn.ffn_layernorm.bias.detach().to(device=dev, dtype=torch.float64)
            pl.w2g = (w2 * g[None, :]).to(act).contiguous()
            pl.c2 = pl.w2g.double().sum(1).float().contiguous()
            pl.d2 = (w2 @ be + ffn.fc2.bias.detach().to(device=dev, dtype=torch.float64)).float().contiguous()
            pl.b1_f32 = _f32(ffn.fc1.bias, dev)
        if resid_fusable(E, F):
            # LN(x) . W^T + b = rstd (xb . W^T - mean' c) + d with xb = act(gamma (x - s)): c = W . gamma
            # (W as the GEMM rounds it), d = W . beta + b (csrc/gp_gemm_impl.h, "the residual epilogues")
            def fold(w_act, ln, b):
                wd = w_act.double()
                return ((wd @ ln.weight.detach().to(device=dev, dtype=torch.float64)).float().contiguous(),
                        (wd @ ln.bias.detach().to(device=dev, dtype=torch.float64) + b.double()).float().contiguous())
            pl.c_qkv, pl.d_qkv = fold(pl.attn.w_qkv, layer.self_attn_layer_norm, pl.attn.b_qkv_f32)
            pl.c1, pl.d1 = fold(pl.w1, layer.final_layer_norm, _f32(ffn.fc1.bias, dev))
        return pl


FFN_FUSED = os.environ.get("GIGAPATH_FFN_FUSED", "1") != "0"
# the residual adds + pre-LNs inside the out-proj / fc2 epilogues and the QKV / fc1 folds (round 4), OFF by
# default since round 6: the round-3 sequence (plain out-proj / fc2 -> gp_residual_layernorm -> plain QKV / fc1)
# is faster in the HIP-graph forward on every measurement (r05: 30.96 / 31.08 / 30.92 vs 30.73 / 30.74 /
# 30.69 ms; r06_base: 29.51 / 29.39 / 29.48 vs 29.38 / 29.27 / 29.06 ms, profiles/r06_base_*) and stays
# inside the north star's 1e-2 at the headline slides (C3 max-rel 8.57e-3, C4 8.14e-3 vs 7.73e-3 / 6.45e-3
# fused, profiles/r06_base_golden_rel_resid_fused_on_off.jsonl).  =1 picks the fused epilogues (more
# parity headroom: the residual stream is rounded once per layer fewer).
RESID_FUSED = os.environ.get("GIGAPATH_RESID_FUSED", "0") == "1"
# the QKV / out-proj / patch projections on gp_linear (own MFMA GEMM, the default) instead of hipBLASLt.
# With every GEMM of the forward on gp_gemm.hip kernels (persistent, data-parallel tiles, no workgroup ever
# waits on another) concurrent HIP-graph replays on several streams run (tests/test_gpu_concurrent.py,
# r03_p: 6.3 s); with hipBLASLt's stream-K QKV / patch GEMMs the same test hung (r03_o, > 180 s).
OWN_GEMMS = os.environ.get("GIGAPATH_OWN_GEMMS", "1") == "1"


def linear(a: torch.Tensor, w: torch.Tensor, b_act: Optional[torch.Tensor], b_f32: Optional[torch.Tensor],
           out: torch.Tensor, gemm_ws: Optional[torch.Tensor] = None, v_bf16: bool = False):
    """out = a . w^T (+ b): nn.Linear on gp_linear when OWN_GEMMS and its instantiations cover the
    shape, else hipBLASLt (torch.addmm / mm).  b_act / b_f32: the bias in the act format / fp32.
    v_bf16: a fused fp16 QKV whose V third is written in bf16 (PackedAttention.v_bf16; own GEMM only)."""
    N, K = w.shape
    if OWN_GEMMS and a.is_cuda and _hip.gemm_supported(N, K) and (b_act is None or b_f32 is not None):
        if gemm_ws is not None and gemm_ws.numel() < _hip.gemm_workspace_bytes(a.shape[0], N, K):
            gemm_ws = None                   # (no split of the last round of tiles)
        # gp_linear's operand contract (row-major, 16-byte aligned rows): a strided or offset caller tensor
        # is copied once instead of being refused
        if not _gemm_rows_ok(a):
            a = a.clone(memory_format=torch.contiguous_format)
        if _gemm_rows_ok(out):
            _hip.linear(a, w, b_f32, out, gemm_ws, v_bf16=v_bf16)
        else:
            tmp = torch.empty(out.shape, dtype=out.dtype, device=out.device)
            _hip.linear(a, w, b_f32, tmp, gemm_ws, v_bf16=v_bf16)
            out.copy_(tmp)
    else:
        if v_bf16:
            raise RuntimeError("runtime.linear: a bf16 V third needs the own GEMM (OWN_GEMMS and a covered shape)")
        with blaslt_serialized():
            if b_act is not None:
                torch.addmm(b_act, a, w.t(), out=out)
            else:
                torch.mm(a, w.t(), out=out)


def _gemm_rows_ok(t: torch.Tensor) -> bool:
    """gp_linear's layout: row-major rows (unit column stride), rows a multiple of 8 elements apart,
    a 16-byte aligned base."""
    return t.dim() == 2 and t.stride(1) == 1 and t.stride(0) % 8 == 0 and t.data_ptr() % 16 == 0


# hipBLASLt GEMMs (shapes outside the own kernels, GIGAPATH_OWN_GEMMS=0 / GIGAPATH_FFN_FUSED=0): its tuned
# stream-K kernels spin on flags of peer workgroups, and concurrent forwards / graph replays on several
# streams hung with them (r03_o).  Every such GEMM issued outside a capture is ordered after
# the previous one on ANY stream of the device (an event chain, no host sync), and a captured graph that
# contains one (BLASLT_ISSUED moved during its capture) replays under the same chain
# (LongNetViT._replay): hipBLASLt never runs on two streams at once.
BLASLT_ISSUED = [0]
_BLASLT_LOCK = threading.RLock()
_BLASLT_LAST: Dict[int, torch.cuda.Event] = {}


def capture_uses_blaslt(before: int) -> bool:
    """True when a hipBLASLt GEMM was issued since BLASLT_ISSUED[0] was `before` (a capture's contents)."""
    return BLASLT_ISSUED[0] != before


def replay_graph(graph) -> None:
    """graph.replay() on the current stream; a graph holding hipBLASLt GEMMs (graph.gp_blaslt, set at
    capture) replays in the device's hipBLASLt event chain (blaslt_serialized)."""
    if getattr(graph, "gp_blaslt", False):
        with blaslt_serialized():
            graph.replay()
    else:
        graph.replay()


class blaslt_serialized:
    """Context of one hipBLASLt launch (or one graph replay containing some) on the current stream."""

    def __enter__(self):
        BLASLT_ISSUED[0] += 1
        self._chain = torch.cuda.is_available() and not torch.cuda.is_current_stream_capturing()
        if self._chain:
            _BLASLT_LOCK.acquire()
            self._stream = torch.cuda.current_stream()
            ev = _BLASLT_LAST.get(self._stream.device.index)
            if ev is not None:
                self._stream.wait_event(ev)
        return self

    def __exit__(self, *exc):
        if self._chain:
            try:
                ev = torch.cuda.Event()
                ev.record(self._stream)
                _BLASLT_LAST[self._stream.device.index] = ev
            finally:
                _BLASLT_LOCK.release()
        return False


def ffn_fusable(E: int, F: int) -> bool:
    """The fused FFN kernels cover fc1 [F, E] (K = E) and fc2 [E, F] (K = F)."""
    return (FFN_FUSED and E in _hip.GEMM_K_E and F in _hip.GEMM_K_F and _hip.gemm_supported(F, E)
            and _hip.gemm_supported(E, F))


def resid_fusable(E: int, F: int) -> bool:
    """Every GEMM of the layer on the residual-epilogue / LN-fold kernels: QKV [3E, E], out-proj [E, E],
    fc1 [F, E] with K = E and fc2 [E, F] with K = F (the three registered archs)."""
    return (RESID_FUSED and FFN_FUSED and OWN_GEMMS and E in _hip.GEMM_K_E and F in _hip.GEMM_K_F
            and all(_hip.gemm_supported(n, k) for n, k in ((3 * E, E), (E, E), (F, E), (E, F))))


def resid_buffers(dev, M: int, E: int):
    """(xstats [E/256 + 1, M, 2], shift [2, M]) of the residual epilogues (fp32).  The two shift rows are
    each padded to a multiple of 4 floats, so both start 16-byte aligned (the GEMMs LDS-DMA them)."""
    mp = (M + 3) // 4 * 4
    return (torch.empty((E // 256 + 1) * M * 2, dtype=torch.float32, device=dev),
            torch.empty(2, mp, dtype=torch.float32, device=dev)[:, :M])


# the residual producers (out-proj, fc2) merge the next LayerNorm's statistics themselves (round 5: in their
# split-tail reduce launch, so the 24 row_stats launches of the consumers go away; the result is the same bits)
MERGE_IN_PRODUCER = os.environ.get("GIGAPATH_MERGE_IN_PRODUCER", "1") != "0"


def fused_qkv(pl: "PackedLayer", ws, qkv: torch.Tensor):
    """QKV of a layer after the first: LN1 folded, A = ws.y (the previous fc2's xb); the statistics merge
    (shift[1] -> shift[0]) is the previous fc2's (MERGE_IN_PRODUCER) or done here."""
    pa = pl.attn
    E = pa.E
    _hip.linear_ln(ws.y, pa.w_qkv, ws.xstats, E // 256, pl.c_qkv, pl.d_qkv, pl.ln1_eps, ws.shift[1], ws.shift[0],
                   qkv, ws.gemm_ws, v_bf16=pa.v_bf16, merged=MERGE_IN_PRODUCER)


def fused_post_attention(pl: "PackedLayer", nxt: Optional["PackedLayer"], ws):
    """out-proj + residual, fc1 (+ folded LN2, GELU), fc2 (+ folded ffn LN, residual, the next layer's
    xb) on ws.a (the merge output).  Shift schedule: out-proj reads shift[0] (the row mean of x before it),
    fc1's merge writes shift[1], fc2 reads it; the next QKV maps shift[1] -> shift[0]."""
    pa = pl.attn
    E = pa.E
    mp = MERGE_IN_PRODUCER
    with TIMER.span("gemm_out"):
        _hip.linear_resid(ws.a, pa.w_o, pa.b_o, ws.x, ws.shift[0], pl.ln2_w, ws.y, ws.xstats, ws.gemm_ws,
                          eps_next=pl.ln2_eps if mp else None, s_out=ws.shift[1] if mp else None)
    with TIMER.span("gemm_fc1"):
        _hip.ffn_fc1_gelu_ln(ws.y, pl.w1, ws.xstats, E // 256, pl.c1, pl.d1, pl.ln2_eps, ws.shift[0], ws.shift[1],
                             ws.f, ws.fstats, merged=mp)
    with TIMER.span("gemm_fc2"):
        last = nxt is None
        _hip.ffn_fc2_ln_resid(ws.f, pl.w2g, ws.fstats, pl.c2, pl.d2, pl.fln_eps, ws.x, ws.shift[1],
                              None if last else nxt.ln1_w, ws.y, ws.xstats, ws.gemm_ws,
                              eps_next=None if (last or not mp) else nxt.ln1_eps,
                              s_out=None if (last or not mp) else ws.shift[0])


def ffn_forward(pl: "PackedLayer", a: torch.Tensor, f: torch.Tensor, y: torch.Tensor, fstats, gemm_ws,
                M: int, F: int, timed: bool = True) -> Optional[torch.Tensor]:
    """FeedForwardNetwork.forward (feedforward_network.py:131-142) without its residual: y = FFN(a).
    Returns the bias the residual add still owes (b2 on the unfused path, None when fused).
    timed=False: no TIMER spans of its own (the CLS tail's M = n launches are timed as one cls_tail span and
    must not be counted among the full-size gemm_fc1 / gemm_fc2 launches)."""
    span = TIMER.span if timed else (lambda name: contextlib.nullcontext())
    if pl.ffn_fused and fstats is not None:
        with span("gemm_fc1"):
            _hip.ffn_fc1_gelu(a, pl.w1, pl.b1_f32, f, fstats)
        with span("gemm_fc2"):
            _hip.ffn_fc2_ln(f, pl.w2g, fstats, pl.c2, pl.d2, pl.fln_eps, y, gemm_ws)
        return None
    with span("gemm_fc1"), blaslt_serialized():
        torch.addmm(pl.b1, a, pl.w1.t(), out=f)
    with span("gelu_ln"):
        _hip.gelu_layernorm(f, pl.fln_w, pl.fln_b, pl.fln_eps, f, M, F)
    with span("gemm_fc2"), blaslt_serialized():
        torch.mm(f, pl.w2.t(), out=y)
    return pl.b2


def ffn_buffers(dev, M: int, E: int, F: int):
    """(stats, GEMM workspace) of the fused FFN for M rows, or (None, workspace) when it does not apply."""
    if not (ffn_fusable(E, F) or resid_fusable(E, F)):
        return None, gemm_workspace(dev, M, E, F)
    stats = torch.empty((F // 256 + 1) * M * 2, dtype=torch.float32, device=dev)
    return stats, gemm_workspace(dev, M, E, F)


def gemm_workspace(dev, M: int, E: int, F: int) -> torch.Tensor:
    """Split-K workspace of the own GEMMs of M rows: fc2 (E x F) and, with OWN_GEMMS, QKV / out-proj."""
    nb = 0
    if torch.device(dev).type == "cuda":
        shapes = [(E, F)] + ([(3 * E, E), (E, E)] if OWN_GEMMS else [])
        nb = max([_hip.gemm_workspace_bytes(M, n, k) for n, k in shapes if _hip.gemm_supported(n, k)], default=0)
    return torch.empty(max(nb, 16), dtype=torch.uint8, device=dev)


def param_signature(module: torch.nn.Module) -> tuple:
    return tuple((p.data_ptr(), p._version, p.dtype) for p in module.parameters())


# ------------------------------------------------------------------------------------------
# the dilated attention core (gather + attention + merge + inner LN), shared by the engine
# and by the standalone DilatedAttention module
# ------------------------------------------------------------------------------------------
class AttentionScratch:
    def __init__(self, dev, B: int, L: int, H: int, D: int, segs, ratios, act: torch.dtype = torch.bfloat16):
        self.key = (B, L, H, D, tuple(segs), tuple(ratios), act)
        self.outs, self.lses = [], []
        for sl, r in zip(segs, ratios):
            s, nseg, m = branch_geometry(L, sl, r)
            self.outs.append(torch.empty(B * nseg * m * H * D, dtype=act, device=dev))
            self.lses.append(torch.empty(B * nseg * H * m, dtype=torch.float32, device=dev))


class VarlenScratch:
    """Packed per-branch outputs of several slides (slide-major regions) and the varlen work table
    bound to one qkv buffer (config C5 packing, _hip.VarlenPlan)."""

    def __init__(self, dev, Ls: Sequence[int], H: int, D: int, segs, ratios, qkv: torch.Tensor):
        self.plan = _hip.VarlenPlan(Ls, H, D, segs, ratios)
        self.outs = [torch.empty(n, dtype=qkv.dtype, device=dev) for n in self.plan.o_elems]
        self.lses = [torch.empty(n, dtype=torch.float32, device=dev) for n in self.plan.lse_elems]
        self.plan.bind(qkv, self.outs, self.lses)


def dilated_attention_core(pa: PackedAttention, qkv: torch.Tensor, B: int, L: int, scratch: AttentionScratch,
                           out: torch.Tensor, inner_ln: bool = True, v_bf16: bool = False):
    """qkv: [B*L, 3E] 16-bit (q | k | v; v_bf16: an fp16 qkv whose V third is bf16, see PackedAttention);
    out: [B*L, E] same format = inner_attn_ln(merge(branches)).  With a VarlenScratch (bound to this qkv),
    every packed slide in one launch each."""
    E, H, D = pa.E, pa.H, pa.D
    if isinstance(scratch, VarlenScratch):
        if not pa.prescaled:
            raise RuntimeError("varlen packing needs the pre-scaled q of D = 48")
        with TIMER.span("attn"):
            _hip.dilated_attn_fwd_varlen(scratch.plan, True, v_bf16=v_bf16)
        with TIMER.span("merge"):
            _hip.branch_merge_ln_varlen(scratch.plan, pa.ln_w if inner_ln else None, pa.ln_b if inner_ln else None,
                                        pa.ln_eps, out)
        return
    with TIMER.span("attn"):
        _hip.dilated_attn_fwd(qkv, qkv[:, E:], qkv[:, 2 * E:], 3 * E, B, L, H, D, pa.segs, pa.ratios,
                              scratch.outs, scratch.lses, 0.0, pa.prescaled, v_bf16=v_bf16)
    with TIMER.span("merge"):
        _hip.branch_merge_ln(scratch.outs, scratch.lses, pa.segs, pa.ratios, B, L, H, D,
                             pa.ln_w if inner_ln else None, pa.ln_b if inner_ln else None, pa.ln_eps, out)


class _DilatedAttentionGrad(torch.autograd.Function):
    """merged = merge(gp_dilated_attn_fwd(qkv)) without the inner LN, differentiable: the backward is one
    gp_dilated_attn_bwd call.  The per-branch o / lse are allocated per call and saved -- the
    module's shared AttentionScratch would be overwritten by the next forward."""

    @staticmethod
    def forward(ctx, qkv, B, L, H, D, segs, ratios, prescaled, softmax_scale):
        E = H * D
        qkv = qkv.contiguous()
        dev, act = qkv.device, qkv.dtype
        outs, lses = [], []
        for sl, r in zip(segs, ratios):
            s, nseg, m = branch_geometry(L, sl, r)
            outs.append(torch.empty(B * nseg * m * H * D, dtype=act, device=dev))
            lses.append(torch.empty(B * nseg * H * m, dtype=torch.float32, device=dev))
        merged = torch.empty(B * L, E, dtype=act, device=dev)
        _hip.dilated_attn_fwd(qkv, qkv[:, E:], qkv[:, 2 * E:], 3 * E, B, L, H, D, segs, ratios, outs, lses,
                              softmax_scale, prescaled)
        _hip.branch_merge_ln(outs, lses, segs, ratios, B, L, H, D, None, None, 0.0, merged)
        ctx.save_for_backward(qkv, *outs, *lses)
        ctx.geom = (B, L, H, D, tuple(segs), tuple(ratios), bool(prescaled), float(softmax_scale))
        return merged

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        B, L, H, D, segs, ratios, prescaled, softmax_scale = ctx.geom
        E = H * D
        qkv, rest = ctx.saved_tensors[0], ctx.saved_tensors[1:]
        outs, lses = list(rest[:len(segs)]), list(rest[len(segs):])
        dout = dout.to(qkv.dtype).contiguous()
        dqkv = torch.empty_like(qkv)
        _hip.dilated_attn_bwd(qkv, qkv[:, E:], qkv[:, 2 * E:], 3 * E, B, L, H, D, segs, ratios, outs, lses, dout,
                              dqkv, dqkv[:, E:], dqkv[:, 2 * E:], 3 * E, softmax_scale, prescaled)
        return (dqkv,) + (None,) * 8


def dilated_attention_grad(qkv: torch.Tensor, B: int, L: int, H: int, D: int, segs, ratios, prescaled: bool,
                           softmax_scale: float = 0.0) -> torch.Tensor:
    """qkv [B*L, 3E] 16-bit (q | k | v; with prescaled, q already times D^-0.5 log2 e) -> merged [B*L, E], the LSE
    merge of every dilation branch before inner_attn_ln, with a native backward to qkv.  The branch weights take
    no gradient, as in the reference (dilated_attention.py:119-124)."""
    if qkv.dtype not in _hip.ACT_DTYPES or qkv.dim() != 2 or qkv.shape != (B * L, 3 * H * D):
        raise ValueError("dilated_attention_grad: qkv must be [B*L, 3*H*D] bf16 or fp16, got %s %s"
                         % (tuple(qkv.shape), qkv.dtype))
    return _DilatedAttentionGrad.apply(qkv, B, L, H, D, list(segs), list(ratios), bool(prescaled),
                                       float(softmax_scale))


class _DilatedAttentionVarlenGrad(torch.autograd.Function):
    """_DilatedAttentionGrad for slides packed token-major in one [T, 3E] qkv: one varlen attention launch and one
    varlen merge forward, one gp_dilated_attn_bwd_varlen call backward.  The packed per-branch o / lse
    are allocated per call (a VarlenScratch bound to this qkv) and saved, as there."""

    @staticmethod
    def forward(ctx, qkv, Ls, H, D, segs, ratios):
        qkv = qkv.contiguous()
        scratch = VarlenScratch(qkv.device, Ls, H, D, segs, ratios, qkv)
        merged = torch.empty(qkv.shape[0], H * D, dtype=qkv.dtype, device=qkv.device)
        _hip.dilated_attn_fwd_varlen(scratch.plan, True)
        _hip.branch_merge_ln_varlen(scratch.plan, None, None, 0.0, merged)
        ctx.save_for_backward(qkv, *scratch.outs, *scratch.lses)
        ctx.geom = (tuple(Ls), H, D, tuple(segs), tuple(ratios))
        return merged

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        Ls, H, D, segs, ratios = ctx.geom
        E = H * D
        qkv, rest = ctx.saved_tensors[0], ctx.saved_tensors[1:]
        outs, lses = list(rest[:len(segs)]), list(rest[len(segs):])
        dout = dout.to(qkv.dtype).contiguous()
        dqkv = torch.empty_like(qkv)
        plan = _hip.VarlenBwdPlan(Ls, H, D, segs, ratios).bind(qkv, outs, lses)
        _hip.dilated_attn_bwd_varlen(plan, dout, dqkv, dqkv[:, E:], dqkv[:, 2 * E:], 3 * E)
        return (dqkv,) + (None,) * 5


def dilated_attention_grad_varlen(qkv: torch.Tensor, Ls: Sequence[int], H: int, D: int, segs, ratios) -> torch.Tensor:
    """qkv [T, 3E] 16-bit, the slides of lengths Ls packed token-major (q | k | v, q already times D^-0.5 log2 e)
    -> merged [T, E]: every slide's own dilated_attention_grad (its own segment schedule, no attention across
    slides), with a native backward to qkv.  D = 48, the arch the varlen kernels cover."""
    Ls = [int(x) for x in Ls]
    if D != 48:
        raise ValueError("dilated_attention_grad_varlen: the varlen kernels cover D = 48 (got %d)" % D)
    if not Ls or min(Ls) < 1:
        raise ValueError("dilated_attention_grad_varlen: every slide needs at least one token, got %s" % (Ls,))
    if qkv.dtype not in _hip.ACT_DTYPES or qkv.dim() != 2 or qkv.shape != (sum(Ls), 3 * H * D):
        raise ValueError("dilated_attention_grad_varlen: qkv must be [sum(Ls), 3*H*D] bf16 or fp16, got %s %s"
                         % (tuple(qkv.shape), qkv.dtype))
    return _DilatedAttentionVarlenGrad.apply(qkv, Ls, H, D, list(segs), list(ratios))


# The training FFN's middle: gelu + ffn_layernorm as gp_gelu_layernorm / gp_gelu_layernorm_bwd (saving only the
# pre-activation).  GIGAPATH_TRAIN_FFN_FUSED=0 selects the plain torch composition for A/B runs.
TRAIN_FFN_FUSED = os.environ.get("GIGAPATH_TRAIN_FFN_FUSED", "1") != "0"
GELU_LN_COLS = (3072, 4096, 6144)


class _GeluLayerNormGrad(torch.autograd.Function):
    """y = LayerNorm(round(gelu_erf(h))) w + b as one kernel each way; h is the only activation saved."""

    @staticmethod
    def forward(ctx, h, ln_weight, ln_bias, eps):
        h = h.contiguous()
        dev = h.device
        w32, b32 = _f32(ln_weight, dev), _f32(ln_bias, dev)
        y = torch.empty_like(h)
        _hip.gelu_layernorm(h, w32, b32, float(eps), y, h.shape[0], h.shape[1])
        ctx.save_for_backward(h, w32)
        ctx.eps = float(eps)
        ctx.param_dtypes = (ln_weight.dtype, ln_bias.dtype)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        h, w32 = ctx.saved_tensors
        ours = dy.dtype != h.dtype or not dy.is_contiguous()
        dy = dy.to(h.dtype).contiguous()
        need_h, need_w, need_b = ctx.needs_input_grad[:3]
        dw = db = None
        if need_w or need_b:
            dw = torch.empty(h.shape[1], dtype=torch.float32, device=h.device)
            db = torch.empty_like(dw)
        # dh over dy when dy is ours to overwrite (the cast / contiguous copy above): one [M, F] buffer fewer.
        # autograd's own buffer is left alone (it may have other readers)
        dh = dy if ours else torch.empty_like(h)
        _hip.gelu_layernorm_bwd(h, dy, w32, ctx.eps, dh, dw, db)
        wd, bd = ctx.param_dtypes
        return (dh if need_h else None, dw.to(wd) if need_w else None, db.to(bd) if need_b else None, None)


def gelu_layernorm_grad(h: torch.Tensor, ln_weight: torch.Tensor, ln_bias: torch.Tensor, eps: float) -> torch.Tensor:
    """h [M, F] 16-bit -> y = ffn_layernorm(gelu(h.float()).type_as(h)) in h's format (feedforward_network.py:
    135-138), differentiable in h and the two LayerNorm parameters: forward gp_gelu_layernorm into a fresh y,
    backward one gp_gelu_layernorm_bwd call (fp32 parameter gradients cast to the parameters' dtype)."""
    if h.dtype not in _hip.ACT_DTYPES or h.dim() != 2 or h.shape[1] not in GELU_LN_COLS:
        raise ValueError("gelu_layernorm_grad: h must be [M, F] bf16 or fp16 with F in %s, got %s %s"
                         % (GELU_LN_COLS, tuple(h.shape), h.dtype))
    return _GeluLayerNormGrad.apply(h, ln_weight, ln_bias, eps)


def gelu_layernorm_torch(h: torch.Tensor, ln_weight: torch.Tensor, ln_bias: torch.Tensor, eps: float,
                         activation_dropout: float = 0.0, training: bool = False) -> torch.Tensor:
    """The same function as torch ops under autograd (GIGAPATH_TRAIN_FFN_FUSED=0, widths the kernel does not
    cover, activation dropout): gelu in fp32, rounded to h's format, [dropout,] LayerNorm in fp32, rounded."""
    g = torch.nn.functional.gelu(h.float()).to(h.dtype)
    if activation_dropout > 0:
        g = torch.nn.functional.dropout(g, activation_dropout, training)
    return torch.nn.functional.layer_norm(g.float(), (h.shape[-1],), ln_weight.float(), ln_bias.float(),
                                          eps).to(h.dtype)


def drop_path(x: torch.Tensor, drop_prob: float, training: bool, slide_lens=None) -> torch.Tensor:
    """The reference's DropPath (timm's drop_path, torchscale/component/droppath.py): one Bernoulli(keep) draw per
    batch element, the kept rows scaled by 1 / keep.  With slide_lens, x is a packed [1, T, E] stream and the draws
    are one per slide (drop_path_scale)."""
    if drop_prob == 0.0 or not training:
        return x
    if slide_lens is not None:
        return x * drop_path_scale(1, drop_prob, training, x.device, slide_lens).view(1, -1, 1).to(x.dtype)
    keep = 1.0 - drop_prob
    mask = x.new_empty((x.shape[0],) + (1,) * (x.dim() - 1)).bernoulli_(keep)
    return x * (mask / keep)


# The training path's rows at the model width: residual add + output dropout + drop-path + the LayerNorm that
# follows, as gp_resid_drop_ln_fwd / gp_resid_drop_ln_bwd.  Saved per call: the LN input, ln_w in fp32,
# the drop-path factors and the dropout seed -- no mask, no statistics, no cast copies.
# GIGAPATH_TRAIN_ROWS_FUSED=0 selects the torch composition for A/B runs.
TRAIN_ROWS_FUSED = os.environ.get("GIGAPATH_TRAIN_ROWS_FUSED", "1") != "0"
ROWS_TRAIN_COLS = _hip.ROWS_TRAIN_COLS


def rows_fusable(E: int, p: float = 0.0) -> bool:
    """Whether the fused row kernels run for width E and dropout probability p (p == 1 stays on torch)."""
    return TRAIN_ROWS_FUSED and E in ROWS_TRAIN_COLS and 0.0 <= p < 1.0


_SLIDE_LENS_DEV: "OrderedDict[tuple, torch.Tensor]" = OrderedDict()


def _slide_lens_dev(slide_lens, dev) -> torch.Tensor:
    """The slide lengths as an int64 device vector (a small cache: a step asks 2 * depth times for the same one)."""
    key = (tuple(int(x) for x in slide_lens), str(dev))
    t = _SLIDE_LENS_DEV.get(key)
    if t is None:
        while len(_SLIDE_LENS_DEV) >= 16:
            _SLIDE_LENS_DEV.popitem(last=False)
        t = _SLIDE_LENS_DEV[key] = torch.tensor(key[0], dtype=torch.int64, device=dev)
    return t


def drop_path_slide_factors(S: int, drop_prob: float, dev) -> torch.Tensor:
    """One Bernoulli(keep) draw per slide, in slide order, scaled by 1 / keep: [S] fp32."""
    keep = 1.0 - drop_prob
    return torch.empty(S, dtype=torch.float32, device=dev).bernoulli_(keep) / keep


def drop_path_scale(B: int, drop_prob: float, training: bool, dev, slide_lens=None) -> Optional[torch.Tensor]:
    """drop_path's per-batch-element factor mask / keep as a [B] fp32 vector (the same draw), or None for 1.  With
    slide_lens (a packed [1, T, E] stream) the draws are one per slide and the result is the per-row [T] vector: each
    slide's factor repeated over its rows (rows_per_scale = 1 for the row kernels)."""
    if drop_prob == 0.0 or not training:
        return None
    if slide_lens is not None:
        f = drop_path_slide_factors(len(slide_lens), drop_prob, dev)
        return torch.repeat_interleave(f, _slide_lens_dev(slide_lens, dev), output_size=int(sum(slide_lens)))
    keep = 1.0 - drop_prob
    return torch.empty(B, dtype=torch.float32, device=dev).bernoulli_(keep) / keep


def _dropout_seed(p: float) -> int:
    """One 64-bit draw per call from torch's CPU default generator (no device sync; torch.manual_seed makes a
    step reproducible).  No draw when there is no dropout."""
    return int(torch.empty((), dtype=torch.int64).random_()) if p > 0 else 0


def _own_f32(dr: torch.Tensor):
    """dr as contiguous fp32, and whether the result is a copy of ours to overwrite (the rule of
    _GeluLayerNormGrad.backward: autograd's own buffer is left alone, it may have other readers)."""
    ours = dr.dtype != torch.float32 or not dr.is_contiguous()
    return dr.float().contiguous(), ours


class _ResidDropLnGrad(torch.autograd.Function):
    """(r, a) = (x + s keep y / (1 - p), LayerNorm(r) w + b rounded to y's format): one kernel each way; r is the
    only activation saved."""

    @staticmethod
    def forward(ctx, x32, y16, ln_weight, ln_bias, eps, p, seed, s):
        x32, y16 = x32.contiguous(), y16.contiguous()
        dev = x32.device
        w32, b32 = _f32(ln_weight, dev), _f32(ln_bias, dev)
        r, a = torch.empty_like(x32), torch.empty_like(y16)
        _hip.resid_drop_ln_fwd(x32, y16, s, p, seed, w32, b32, eps, r, a)
        ctx.save_for_backward(r, w32, s)
        ctx.args = (float(eps), float(p), int(seed), y16.dtype)
        ctx.param_dtypes = (ln_weight.dtype, ln_bias.dtype)
        ctx.set_materialize_grads(False)
        return r, a

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dr, da):
        r, w32, s = ctx.saved_tensors
        eps, p, seed, act = ctx.args
        if dr is None and da is None:
            return (None,) * 8
        need_w, need_b = ctx.needs_input_grad[2:4]
        dy = torch.empty(r.shape, dtype=act, device=r.device)
        dw = db = None
        if da is None:
            # a was not used: the add alone (the LayerNorm takes no gradient)
            dx, _ = _own_f32(dr)
            _hip.resid_drop_ln_bwd(None, dx, None, None, eps, s, p, seed, None, dy)
            need_w = need_b = False
        else:
            da = da.to(act).contiguous()
            if need_w or need_b:
                dw = torch.empty(r.shape[1], dtype=torch.float32, device=r.device)
                db = torch.empty_like(dw)
            # dx over dr when dr is ours to overwrite: one [M, E] fp32 buffer fewer
            dr_in, ours = _own_f32(dr) if dr is not None else (None, False)
            dx = dr_in if ours else torch.empty_like(r)
            _hip.resid_drop_ln_bwd(da, dr_in, r, w32, eps, s, p, seed, dx, dy, dw, db)
        wd, bd = ctx.param_dtypes
        return (dx, dy, dw.to(wd) if need_w else None, db.to(bd) if need_b else None, None, None, None, None)


class _ResidDropGrad(torch.autograd.Function):
    """r = x + s keep y / (1 - p): one kernel each way, nothing but s and the seed saved."""

    @staticmethod
    def forward(ctx, x32, y16, p, seed, s):
        x32, y16 = x32.contiguous(), y16.contiguous()
        r = torch.empty_like(x32)
        _hip.resid_drop_ln_fwd(x32, y16, s, p, seed, None, None, 0.0, r, None)
        ctx.save_for_backward(s)
        ctx.args = (float(p), int(seed), y16.dtype)
        return r

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dr):
        (s,) = ctx.saved_tensors
        p, seed, act = ctx.args
        dx, _ = _own_f32(dr)
        dy = torch.empty(dx.shape, dtype=act, device=dx.device)
        _hip.resid_drop_ln_bwd(None, dx, None, None, 0.0, s, p, seed, None, dy)
        return dx, dy, None, None, None


class _LayerNormActGrad(torch.autograd.Function):
    """a = LayerNorm(x) w + b rounded to the 16-bit format, x fp32 or 16-bit: one kernel each way; x and ln_w in
    fp32 are saved."""

    @staticmethod
    def forward(ctx, x, ln_weight, ln_bias, eps, act):
        x = x.contiguous()
        dev = x.device
        w32, b32 = _f32(ln_weight, dev), _f32(ln_bias, dev)
        a = torch.empty(x.shape, dtype=act, device=dev)
        _hip.resid_drop_ln_fwd(x, None, None, 0.0, 0, w32, b32, eps, None, a)
        ctx.save_for_backward(x, w32)
        ctx.args = (float(eps), act)
        ctx.param_dtypes = (ln_weight.dtype, ln_bias.dtype)
        return a

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, da):
        x, w32 = ctx.saved_tensors
        eps, act = ctx.args
        da = da.to(act).contiguous()
        need_w, need_b = ctx.needs_input_grad[1:3]
        dw = db = None
        if need_w or need_b:
            dw = torch.empty(x.shape[1], dtype=torch.float32, device=x.device)
            db = torch.empty_like(dw)
        dx = torch.empty_like(x)
        _hip.resid_drop_ln_bwd(da, None, x, w32, eps, None, 0.0, 0, dx, None, dw, db)
        wd, bd = ctx.param_dtypes
        return (dx, dw.to(wd) if need_w else None, db.to(bd) if need_b else None, None, None)


def _rows_check(who: str, x: torch.Tensor, y: Optional[torch.Tensor]):
    if x.dim() != 2 or x.shape[1] not in ROWS_TRAIN_COLS:
        raise ValueError("%s: x must be [M, E] with E in %s, got %s" % (who, ROWS_TRAIN_COLS, tuple(x.shape)))
    if y is not None and (x.dtype != torch.float32 or y.dtype not in _hip.ACT_DTYPES or y.shape != x.shape):
        raise ValueError("%s: x must be fp32 and y bf16 or fp16 of x's shape, got %s %s and %s %s"
                         % (who, tuple(x.shape), x.dtype, tuple(y.shape), y.dtype))


def _rows_torch_add(x32, y16, p, scale, training):
    """Today's lines (encoder.py): dropout in fp32, drop-path, residual add."""
    a = torch.nn.functional.dropout(y16.float(), p, training)
    if scale is not None:
        a = (a.view(scale.numel(), -1) * scale.view(-1, 1)).view_as(a)
    return x32 + a


def _ln_torch(x: torch.Tensor, ln, act: torch.dtype) -> torch.Tensor:
    return torch.nn.functional.layer_norm(x.float(), (x.shape[-1],), ln.weight.float(), ln.bias.float(),
                                          ln.eps).to(act)


def resid_drop_ln_grad(x32: torch.Tensor, y16: torch.Tensor, ln, p: float, scale: Optional[torch.Tensor],
                       training: bool):
    """x32 [M, E] fp32 residual stream, y16 [M, E] 16-bit branch output, ln an nn.LayerNorm(E), p the output dropout
    probability (applied when training), scale the drop-path factors of drop_path_scale ([B], M = B L) or None
    -> (r32, a16): r = x + drop_path(dropout(y)) in fp32 and a = ln(r) rounded to y's format, differentiable in x,
    y and the two LayerNorm parameters: one gp_resid_drop_ln_fwd call forward, one gp_resid_drop_ln_bwd call
    backward (fp32 parameter gradients cast to the parameters' dtype).  The torch composition runs with
    GIGAPATH_TRAIN_ROWS_FUSED=0, at other widths and at p == 1."""
    p = float(p) if training else 0.0
    if not rows_fusable(x32.shape[-1], p):
        r = _rows_torch_add(x32, y16, p, scale, training)
        return r, _ln_torch(r, ln, y16.dtype)
    _rows_check("resid_drop_ln_grad", x32, y16)
    return _ResidDropLnGrad.apply(x32, y16, ln.weight, ln.bias, float(ln.eps), p, _dropout_seed(p), scale)


def resid_drop_grad(x32: torch.Tensor, y16: torch.Tensor, p: float, scale: Optional[torch.Tensor],
                    training: bool) -> torch.Tensor:
    """resid_drop_ln_grad without the LayerNorm: r32 alone."""
    p = float(p) if training else 0.0
    if not rows_fusable(x32.shape[-1], p):
        return _rows_torch_add(x32, y16, p, scale, training)
    _rows_check("resid_drop_grad", x32, y16)
    return _ResidDropGrad.apply(x32, y16, p, _dropout_seed(p), scale)


def layernorm_act_grad(x: torch.Tensor, ln, act: Optional[torch.dtype] = None) -> torch.Tensor:
    """x [M, E] fp32 (the residual stream) or 16-bit -> ln(x) rounded to the 16-bit format (x's own; for an fp32 x,
    act or the call's activation format), differentiable in x and the LayerNorm parameters."""
    act = x.dtype if x.dtype in _hip.ACT_DTYPES else (act or act_dtype())
    if not rows_fusable(x.shape[-1]):
        return _ln_torch(x, ln, act)
    _rows_check("layernorm_act_grad", x, None)
    if x.dtype != torch.float32 and x.dtype not in _hip.ACT_DTYPES:
        raise ValueError("layernorm_act_grad: x must be fp32, bf16 or fp16, got %s" % x.dtype)
    return _LayerNormActGrad.apply(x, ln.weight, ln.bias, float(ln.eps), act)


def takes_grad_path(module: torch.nn.Module, *inputs) -> bool:
    """The opt-in rule of the trainable modules: the module's `trainable` flag, grad mode on, and an input that
    requires grad or .train() with a parameter that does."""
    if not getattr(module, "trainable", False) or not torch.is_grad_enabled():
        return False
    if any(isinstance(t, torch.Tensor) and t.requires_grad for t in inputs):
        return True
    return module.training and any(p.requires_grad for p in module.parameters())


# ------------------------------------------------------------------------------------------
# encoder engine
# ------------------------------------------------------------------------------------------
class ClsRows:
    """Buffers of the last layer's CLS tail (EncoderEngine.run_layers cls_rows=): n = one row per slide.
    off / len: [n] int64 device tensors, the row of each slide's token 0 in the workspace and its length
    (gp_cls_attn_merge_ln's slide_off / slide_len; also the gather index of the CLS rows of ws.x).  They and
    every buffer here live as long as the workspace that owns them: a HIP graph bakes their pointers."""

    def __init__(self, dev, offs: Sequence[int], lens: Sequence[int], E: int, F: int, H: int, segs, ratios,
                 act: torch.dtype):
        n = len(offs)
        self.n, self.max_len = n, int(max(lens))
        self.off = torch.tensor([int(o) for o in offs], dtype=torch.int64, device=dev)
        self.len = torch.tensor([int(l) for l in lens], dtype=torch.int64, device=dev)
        self.x = torch.empty(n, E, dtype=torch.float32, device=dev)      # the CLS rows of the residual stream
        self.a = torch.empty(n, E, dtype=act, device=dev)                # inner_attn_ln(merge), then LN2(x1)
        self.y = torch.empty(n, E, dtype=act, device=dev)                # out-proj output
        self.y2 = torch.empty(n, E, dtype=act, device=dev)               # fc2 output
        self.f = torch.empty(n, F, dtype=act, device=dev)
        self.fstats, self.gemm_ws = ffn_buffers(dev, n, E, F)
        self.attn_ws = torch.empty(_hip.cls_attn_workspace_bytes(self.max_len, n, H, E // H, segs, ratios),
                                   dtype=torch.uint8, device=dev)


def key_row_plan(L: int, segs: Sequence[int], ratios: Sequence[int]):
    """The tokens whose K / V the CLS query of a slide of L tokens reads: branch (sl, r) with
    s = min(sl, L), m = ceil(s / r) attends tokens 0, r, ..., (m - 1) r.  Returns (rows, row_map, groups):
      rows     sorted int32 array S, the union over the branches;
      row_map  int32 [L]: row_map[S[k]] = k, -1 for a token outside S;
      groups   per branch (off, idx): the sparse rows the merge reads for the tokens of S.  Token p comes from
               sparse row i of (segment n, head group j) with p = n g + i r + j, g = m r (sparse_to_dense,
               dilated_attention.py:33-53; g = s, so p is that row's own query token, wherever r divides s or the
               branch has one segment); idx[off[n r + j] : off[n r + j + 1]] lists the i of that group, ascending."""
    L = int(L)
    mark = np.zeros(L, dtype=bool)
    for sl, r in zip(segs, ratios):
        s, _, m = branch_geometry(L, sl, r)
        mark[np.arange(m, dtype=np.int64) * r] = True
    rows = np.flatnonzero(mark).astype(np.int32)
    row_map = np.full(L, -1, dtype=np.int32)
    row_map[rows] = np.arange(rows.size, dtype=np.int32)
    groups = []
    t = rows.astype(np.int64)
    for sl, r in zip(segs, ratios):
        s, nseg, m = branch_geometry(L, sl, r)
        n, w = t // (m * r), t % (m * r)
        g = n * r + w % r
        order = np.argsort(g, kind="stable")           # (tokens ascend within a group, so i does)
        off = np.zeros(nseg * r + 1, dtype=np.int32)
        np.cumsum(np.bincount(g, minlength=nseg * r), out=off[1:])
        groups.append((off, (w // r)[order].astype(np.int32)))
    return rows, row_map, groups


class KeyRows:
    """Buffers of the key-row tail (EncoderEngine.key_row_tail): the second-to-last layer after its attention, and
    the last layer's QKV GEMM, on the n = |S| rows per slide that the CLS tail reads (key_row_plan).  One list for
    every slide of the [B, L] batch; slide b's rows are compact rows [b n, (b + 1) n), its CLS first.  Everything
    here is fixed by the workspace key and lives as long as the workspace: a HIP graph bakes the pointers."""

    def __init__(self, dev, B: int, L: int, E: int, F: int, plan, act: torch.dtype):
        rows, row_map, self.groups = plan
        self._attn_plan = None
        n = int(rows.size)
        self.n, self.M = n, B * n
        self.rows = torch.from_numpy(rows).to(dev)                       # [n] int32: the tokens S
        self.row_map = torch.from_numpy(row_map).to(dev)                 # [L] int32: token -> compact row
        gather = (np.arange(B, dtype=np.int64)[:, None] * L + rows.astype(np.int64)[None, :]).reshape(-1)
        self.gather = torch.from_numpy(gather).to(dev)                   # [B n] int64: rows of ws.x
        self.off = torch.arange(B, dtype=torch.int64, device=dev) * n    # each slide's first compact row (its CLS)
        M = self.M
        self.x = torch.empty(M, E, dtype=torch.float32, device=dev)
        self.a = torch.empty(M, E, dtype=act, device=dev)
        self.y = torch.empty(M, E, dtype=act, device=dev)
        self.y2 = torch.empty(M, E, dtype=act, device=dev)
        self.f = torch.empty(M, F, dtype=act, device=dev)
        self.qkv = torch.empty(M, 3 * E, dtype=act, device=dev)          # the last layer's (V third: see Workspace)
        self.fstats, self.gemm_ws = ffn_buffers(dev, M, E, F)

    def attn_rows_plan(self, ws, pa: "PackedAttention", B: int, L: int):
        """The query-list attention's work table bound to ws.qkv and ws.attn (built once), or None where the
        list launch does not cover the call: a q that is not pre-scaled, or fp16 with an fp16 V (the exact
        running-max kernel has no list variant); the full launch then runs."""
        if not pa.prescaled or pa.D != 48 or (ws.qkv.dtype == torch.float16 and not pa.v_bf16):
            return None
        if self._attn_plan is None:
            self._attn_plan = _hip.AttnRowsPlan(ws.qkv, B, L, pa.H, pa.D, pa.segs, pa.ratios, self.groups,
                                                ws.attn.outs, ws.attn.lses)
        return self._attn_plan


class Workspace:
    cls: Optional[ClsRows] = None
    _key_rows = None        # unset; False: the key-row tail does not apply at this shape

    def key_rows(self) -> Optional[KeyRows]:
        """The key-row tail's buffers (built on first use), or None where it does not engage: more than
        KEYROW_MAX_SHARE of the rows are needed, or gp_branch_merge_ln_rows does not cover the shape."""
        if self._key_rows is None:
            self._key_rows = False
            B, L, E, F, H = self.key[1:6]
            segs, ratios, act = self.key[-3], self.key[-2], self.key[-1]
            if _hip.branch_merge_ln_rows_supported(H, E // H, len(segs)):
                plan = key_row_plan(L, segs, ratios)
                if plan[0].size <= KEYROW_MAX_SHARE * L:
                    self._key_rows = KeyRows(self.x.device, B, L, E, F, plan, act)
        return self._key_rows or None

    def cls_rows(self) -> ClsRows:
        """The CLS tail's buffers, allocated on first use (an eager run precedes every graph capture)."""
        if self.cls is None:
            dev, E, F = self.x.device, self.x.shape[1], self.f.shape[1]
            segs, ratios, act = self.key[-3], self.key[-2], self.key[-1]
            H = self.key[-4]
            offs, lens = self._slides()
            self.cls = ClsRows(dev, offs, lens, E, F, H, segs, ratios, act)
        return self.cls

    def _slides(self):
        B, L = self.key[1], self.key[2]
        return [b * L for b in range(B)], [L] * B

    def __init__(self, dev, B: int, L: int, E: int, F: int, H: int, segs, ratios, act: torch.dtype = torch.bfloat16):
        M = B * L
        self.key = (str(dev), B, L, E, F, H, tuple(segs), tuple(ratios), act)
        self.x = torch.empty(M, E, dtype=torch.float32, device=dev)
        self.a = torch.empty(M, E, dtype=act, device=dev)
        # fused q | k | v; NOTE under the fp16 caller (PackedAttention.v_bf16) the V third holds bf16 bits
        # although the tensor is fp16: read it through PackedAttention.qkv_parts
        self.qkv = torch.empty(M, 3 * E, dtype=act, device=dev)
        self.y = torch.empty(M, E, dtype=act, device=dev)
        self.y2 = torch.empty(M, E, dtype=act, device=dev)     # fc2 output (y keeps the out-proj's: RESID2)
        self.f = torch.empty(M, F, dtype=act, device=dev)
        self.fstats, self.gemm_ws = ffn_buffers(dev, M, E, F)
        self.xstats, self.shift = resid_buffers(dev, M, E)
        self.attn = AttentionScratch(dev, B, L, H, E // H, segs, ratios, act)


class PackedWorkspace(Workspace):
    """Workspace of several slides packed token-major: T = sum(L_i) rows, slide i at rows
    [tok_off[i], tok_off[i] + L_i) with its CLS first; attention through a VarlenScratch."""

    def __init__(self, dev, Ls: Sequence[int], E: int, F: int, H: int, segs, ratios,
                 act: torch.dtype = torch.bfloat16):
        self.Ls = [int(x) for x in Ls]
        T = sum(self.Ls)
        M = T
        self.key = (str(dev), tuple(self.Ls), E, F, H, tuple(segs), tuple(ratios), act)
        self.x = torch.empty(M, E, dtype=torch.float32, device=dev)
        self.a = torch.empty(M, E, dtype=act, device=dev)
        self.qkv = torch.empty(M, 3 * E, dtype=act, device=dev)   # (V third: see Workspace, qkv_parts)
        self.y = torch.empty(M, E, dtype=act, device=dev)
        self.y2 = torch.empty(M, E, dtype=act, device=dev)
        self.f = torch.empty(M, F, dtype=act, device=dev)
        self.fstats, self.gemm_ws = ffn_buffers(dev, M, E, F)
        self.xstats, self.shift = resid_buffers(dev, M, E)
        self.attn = VarlenScratch(dev, self.Ls, H, E // H, segs, ratios, self.qkv)
        self.tok_off = self.attn.plan.tok_off
        self.cls_idx = torch.tensor(self.tok_off[:-1], dtype=torch.int64, device=dev)

    def _slides(self):
        return self.tok_off[:-1], self.Ls

    def key_rows(self):
        return None          # (the packed forward keeps the full second-to-last layer)


class EncoderEngine:
    """Runs the 12-layer (or 24-) LongNet stack on one device for inputs already embedded."""

    def __init__(self):
        self._sig = None
        self.layers: List[PackedLayer] = []
        self._packs: Dict[torch.dtype, tuple] = {}     # act -> (signature, packed layers)
        # activation workspaces per CALLER STREAM: two streams never share activation buffers, so
        # forwards issued on different streams can run concurrently; ws / pws = the last one used.
        # LRU-bounded (max_stream_workspaces): a caller using a fresh stream per request does not grow
        # them without limit.  A HIP graph's workspace is detached from these maps after its capture
        # (detach_workspace) and lives exactly as long as the graph (LongNetViT._graph_ws).
        self._ws: "OrderedDict[int, Workspace]" = OrderedDict()
        self._pws: "OrderedDict[int, PackedWorkspace]" = OrderedDict()
        self.ws: Optional[Workspace] = None
        self.pws: Optional[PackedWorkspace] = None

    def pack(self, encoder, dev, act: Optional[torch.dtype] = None):
        """Packed layers for the activation format `act` (default: the current call's, act_dtype());
        one packing per format is kept, so alternating bf16 / fp16 callers do not repack."""
        use_tuned_gemms(dev)
        act = act or act_dtype()
        sig = (str(dev), param_signature(encoder), act)
        ent = self._packs.get(act)
        if ent is None or ent[0] != sig:
            ent = (sig, [PackedLayer.from_module(l, dev, act) for l in encoder.layers])
            self._packs[act] = ent
        self._sig, self.layers = ent
        return self.layers

    @staticmethod
    def _stream_key(dev) -> int:
        return int(torch.cuda.current_stream(dev).cuda_stream) if torch.device(dev).type == "cuda" else 0

    # (8 = LongNetViT.max_capture_streams: the documented 4-stream concurrent pattern plus the default stream
    # and the capture side streams stay cached; beyond it an eager call on yet another stream evicts the least
    # recently used workspace and reallocates its own -- correct, but hundreds of MB per call at 20-70k tiles)
    max_stream_workspaces = 8

    def _cached(self, table, key, make):
        sk = self._stream_key(self._dev_of(key))
        ws = table.get(sk)
        if ws is None or ws.key != key:
            table.pop(sk, None)                # (a HIP graph that baked the old one keeps it alive)
            while len(table) >= self.max_stream_workspaces:
                old = next(iter(table))        # least recently used caller stream
                table.pop(old)
            ws = table[sk] = make()
        table.move_to_end(sk)
        return ws

    @staticmethod
    def _dev_of(key):
        return torch.device(key[0])

    def workspace(self, dev, B, L, E, F, H, segs, ratios, act: Optional[torch.dtype] = None) -> Workspace:
        act = act or act_dtype()
        key = (str(dev), B, L, E, F, H, tuple(segs), tuple(ratios), act)
        self.ws = self._cached(self._ws, key, lambda: Workspace(dev, B, L, E, F, H, segs, ratios, act))
        return self.ws

    def workspace_packed(self, dev, Ls, E, F, H, segs, ratios, act: Optional[torch.dtype] = None) -> PackedWorkspace:
        act = act or act_dtype()
        key = (str(dev), tuple(int(x) for x in Ls), E, F, H, tuple(segs), tuple(ratios), act)
        self.pws = self._cached(self._pws, key, lambda: PackedWorkspace(dev, Ls, E, F, H, segs, ratios, act))
        return self.pws

    def stream_workspace(self, stream, packed: bool = False):
        """The workspace the engine keeps for `stream` (the one a forward issued on that stream used),
        or None."""
        table = self._pws if packed else self._ws
        return table.get(int(stream.cuda_stream)) if stream is not None else None

    def detach_workspace(self, ws) -> None:
        """Forget `ws` (a HIP graph's baked workspace): the next eager call on its stream allocates a new
        one, and the graph cache alone decides how long `ws` lives."""
        for table in (self._ws, self._pws):
            for k in [k for k, v in table.items() if v is ws]:
                table.pop(k)
        if self.ws is ws:
            self.ws = None
        if self.pws is ws:
            self.pws = None

    def _resid_fused_path(self, ws) -> bool:
        return bool(self.layers) and all(pl.resid_fused for pl in self.layers) and ws.fstats is not None

    def key_row_tail(self, ws, cls_rows: Optional[ClsRows]) -> Optional[KeyRows]:
        """The KeyRows run_layers(ws, ..., cls_rows=cls_rows) runs the second-to-last layer on, or None: that
        layer's output feeds only the last layer's K / V rows of the CLS query's keys and the CLS readout, so
        with the CLS tail on it runs for those rows alone.  Not on the packed forward, the
        residual-epilogue path, models of fewer than 3 layers, or where Workspace.key_rows() declines.  When
        taken, ws.x keeps the output of layer depth-3 and layer depth-2's output is KeyRows.x (slide b's CLS at
        row KeyRows.off[b])."""
        if cls_rows is None or not KEYROW_TAIL or len(self.layers) < 3 or self._resid_fused_path(ws):
            return None
        return ws.key_rows()

    def run_layers(self, ws: Workspace, B: int, L: int, layer_hook=None, shift_ready: bool = False,
                   cls_rows: Optional[ClsRows] = None):
        """ws.x holds the fp32 embedding and ws.a = LN1_0(ws.x) (16-bit).  Runs every layer in
        place; layer_hook(i) is called after layer i-1 finishes (i = 1..depth).  shift_ready: ws.shift[0]
        already holds the row means of ws.x (gp_posembed_cls_ln's row_mean); otherwise they are computed.
        cls_rows (ws.cls_rows()): the caller reads only the CLS row of each slide from the LAST layer's
        output, so that layer runs its QKV GEMM and then cls_tail() on one row per slide; its output is
        cls_rows.x, and ws.x keeps the second-to-last layer's.  None: every layer in full."""
        M = B * L
        E = ws.x.shape[1]
        F = ws.f.shape[1]
        nl = len(self.layers)
        if self._resid_fused_path(ws):
            if not shift_ready:
                torch.mean(ws.x, 1, out=ws.shift[0])
            for li, pl in enumerate(self.layers):
                pa = pl.attn
                with TIMER.span("gemm_qkv"):
                    if li == 0:
                        linear(ws.a, pa.w_qkv, pa.b_qkv, pa.b_qkv_f32, ws.qkv, ws.gemm_ws, v_bf16=pa.v_bf16)
                    else:
                        fused_qkv(pl, ws, ws.qkv)
                if cls_rows is not None and li + 1 == nl:
                    cls_tail(pl, ws, cls_rows)
                else:
                    dilated_attention_core(pa, ws.qkv, B, L, ws.attn, ws.a, v_bf16=pa.v_bf16)
                    fused_post_attention(pl, self.layers[li + 1] if li + 1 < nl else None, ws)
                if layer_hook is not None:
                    layer_hook(li + 1)
            return
        kr = self.key_row_tail(ws, cls_rows)
        for li, pl in enumerate(self.layers):
            pa = pl.attn
            if cls_rows is not None and li + 1 == nl:
                if kr is not None:
                    with TIMER.span("keyrow_tail"):
                        linear(kr.a, pa.w_qkv, pa.b_qkv, pa.b_qkv_f32, kr.qkv, kr.gemm_ws, v_bf16=pa.v_bf16)
                else:
                    with TIMER.span("gemm_qkv"):
                        linear(ws.a, pa.w_qkv, pa.b_qkv, pa.b_qkv_f32, ws.qkv, ws.gemm_ws, v_bf16=pa.v_bf16)
                cls_tail(pl, ws, cls_rows, kr)
                if layer_hook is not None:
                    layer_hook(li + 1)
                continue
            with TIMER.span("gemm_qkv"):
                linear(ws.a, pa.w_qkv, pa.b_qkv, pa.b_qkv_f32, ws.qkv, ws.gemm_ws, v_bf16=pa.v_bf16)
            if kr is not None and li + 2 == nl:
                key_row_layer(pl, self.layers[li + 1], ws, kr, B, L)
                if layer_hook is not None:
                    layer_hook(li + 1)
                continue
            dilated_attention_core(pa, ws.qkv, B, L, ws.attn, ws.a, v_bf16=pa.v_bf16)
            with TIMER.span("gemm_out"):
                linear(ws.a, pa.w_o, None, None, ws.y, ws.gemm_ws)
            nxt = self.layers[li + 1] if li + 1 < nl else None
            residual_pair(pl, nxt, ws, M, E, F)
            if layer_hook is not None:
                layer_hook(li + 1)


# the layer's two residual adds as gp_residual2_layernorm (round 6): the first leaves x unwritten, the second
# recomputes x1 from x and the out-proj output y and adds the fc2 output -- 22 instead of 24 bytes per element,
# bit-identical to the two gp_residual_layernorm passes (=0 restores those)
RESID2 = os.environ.get("GIGAPATH_RESID2", "1") != "0"


def residual_pair(pl: "PackedLayer", nxt: Optional["PackedLayer"], ws, M: int, E: int, F: int):
    """The unfused layer tail after the out-proj GEMM wrote ws.y: residual + LN2, FFN, residual + the next
    layer's LN1 (encoder.py:141-162)."""
    pa = pl.attn
    ln1 = (nxt.ln1_w, nxt.ln1_b, nxt.ln1_eps) if nxt else (None, None, 1e-5)
    if RESID2:
        with TIMER.span("resid_ln"):
            _hip.residual2_layernorm(ws.x, ws.y, pa.b_o, None, None, pl.ln2_w, pl.ln2_b, pl.ln2_eps, ws.a, M, E)
        b2 = ffn_forward(pl, ws.a, ws.f, ws.y2, ws.fstats, ws.gemm_ws, M, F)
        with TIMER.span("resid_ln"):
            _hip.residual2_layernorm(ws.x, ws.y, pa.b_o, ws.y2, b2, ln1[0], ln1[1], ln1[2], ws.a, M, E)
        return
    with TIMER.span("resid_ln"):
        _hip.residual_layernorm(ws.x, ws.y, pa.b_o, pl.ln2_w, pl.ln2_b, pl.ln2_eps, ws.a, M, E)
    b2 = ffn_forward(pl, ws.a, ws.f, ws.y, ws.fstats, ws.gemm_ws, M, F)
    with TIMER.span("resid_ln"):
        _hip.residual_layernorm(ws.x, ws.y, b2, ln1[0], ln1[1], ln1[2], ws.a, M, E)


# the last layer for the CLS rows only (cls_tail) when the readout is the CLS token (LongNetViT with
# global_pool off).  =0 restores the full last layer (A/B runs, tests/test_gpu_cls_tail.py).
CLS_TAIL = os.environ.get("GIGAPATH_CLS_TAIL", "1") != "0"


# the second-to-last layer for the rows the CLS tail reads (key_row_layer).  =0 restores the full layer; means
# nothing unless the CLS tail is on.
KEYROW_TAIL = os.environ.get("GIGAPATH_KEYROW_TAIL", "1") != "0"
# engaged where at most this share of a slide's rows is needed (|S| <= L / 2: L >= 7,842 on the product schedule;
# below it tests/test_gpu_cls_tail.py's on / off bit-identity of the earlier layers holds by not engaging)
KEYROW_MAX_SHARE = 0.5


def key_row_layer(pl: "PackedLayer", nxt: "PackedLayer", ws, kr: KeyRows, B: int, L: int):
    """Encoder layer depth-2 after its QKV GEMM wrote ws.qkv, for the rows kr.rows of every slide: the attention
    of the sparse rows their merge reads (gp_dilated_attn_fwd_rows; every key is still attended to), then the
    branch merge + inner LN of the listed tokens into the compact kr.a and EncoderLayer.forward's remaining steps (encoder.py:141-162) at M = B |S| on
    kr's buffers, as residual_pair runs them.  Leaves kr.x (the layer's output rows) and kr.a = the last layer's
    LN1 of them; ws.x keeps the layer's input."""
    pa = pl.attn
    E, F, M = pa.E, kr.f.shape[1], kr.M
    plan = kr.attn_rows_plan(ws, pa, B, L)
    if plan is not None:
        with TIMER.span("keyrow_attn"):
            _hip.dilated_attn_fwd_rows(plan, True, v_bf16=pa.v_bf16)
    else:
        with TIMER.span("attn"):
            _hip.dilated_attn_fwd(ws.qkv, ws.qkv[:, E:], ws.qkv[:, 2 * E:], 3 * E, B, L, pa.H, pa.D, pa.segs,
                                  pa.ratios, ws.attn.outs, ws.attn.lses, 0.0, pa.prescaled, v_bf16=pa.v_bf16)
    with TIMER.span("keyrow_merge"):
        _hip.branch_merge_ln_rows(ws.attn.outs, ws.attn.lses, pa.segs, pa.ratios, B, L, kr.rows, pa.H, pa.D,
                                  pa.ln_w, pa.ln_b, pa.ln_eps, kr.a)
    with TIMER.span("keyrow_tail"):
        torch.index_select(ws.x, 0, kr.gather, out=kr.x)
        linear(kr.a, pa.w_o, None, None, kr.y, kr.gemm_ws)
        _hip.residual2_layernorm(kr.x, kr.y, pa.b_o, None, None, pl.ln2_w, pl.ln2_b, pl.ln2_eps, kr.a, M, E)
        b2 = ffn_forward(pl, kr.a, kr.f, kr.y2, kr.fstats, kr.gemm_ws, M, F, timed=False)
        _hip.residual2_layernorm(kr.x, kr.y, pa.b_o, kr.y2, b2, nxt.ln1_w, nxt.ln1_b, nxt.ln1_eps, kr.a, M, E)


def cls_tail(pl: "PackedLayer", ws, c: ClsRows, kr: Optional[KeyRows] = None):
    """The last encoder layer after its QKV GEMM wrote ws.qkv, for the CLS token of every slide: the row the
    readout outcome = self.norm(x)[:, 0] (slide_encoder.py:213-221) takes from that layer.  The CLS query's
    attention, branch merge and inner LN in gp_cls_attn_merge_ln (K / V of every token it attends to come from
    ws.qkv), then EncoderLayer.forward's remaining steps (encoder.py:141-162) at M = n rows on c's buffers:
    out-proj, residual + LN2, FFN, residual.  Result: c.x [n, E] fp32.  kr (the key-row tail): the layer's qkv and
    input rows are the compact kr.qkv / kr.x, token t of slide b at row kr.off[b] + kr.row_map[t]."""
    pa = pl.attn
    n, E, F = c.n, pa.E, c.f.shape[1]
    qkv, x, off = (ws.qkv, ws.x, c.off) if kr is None else (kr.qkv, kr.x, kr.off)
    q, k, v = qkv, qkv[:, E:], qkv[:, 2 * E:]
    with TIMER.span("cls_attn"):
        _hip.cls_attn_merge_ln(q, k, v, 3 * E, off, c.len, c.max_len, pa.H, pa.D, pa.segs, pa.ratios, pa.ln_w,
                               pa.ln_b, pa.ln_eps, c.a, c.attn_ws, 0.0, pa.prescaled, v_bf16=pa.v_bf16,
                               row_map=None if kr is None else kr.row_map, map_rows=0 if kr is None else kr.n)
    with TIMER.span("cls_tail"):
        torch.index_select(x, 0, off, out=c.x)
        linear(c.a, pa.w_o, None, None, c.y, c.gemm_ws)
        _hip.residual2_layernorm(c.x, c.y, pa.b_o, None, None, pl.ln2_w, pl.ln2_b, pl.ln2_eps, c.a, n, E)
        b2 = ffn_forward(pl, c.a, c.f, c.y2, c.fstats, c.gemm_ws, n, F, timed=False)
        _hip.residual2_layernorm(c.x, c.y, pa.b_o, c.y2, b2, None, None, 1e-5, c.a, n, E)


def gemm_flops(B: int, N: int, E: int, F: int, C: int, depth: int) -> float:
    L = N + 1
    return float(2 * B * L * (4 * E * E + 2 * E * F) * depth + 2 * B * N * C * E)


def merge_bytes(L: int, segs: Sequence[int], ratios: Sequence[int], H: int, D: int, B: int = 1) -> float:
    """Algorithmic HBM bytes of one gp_branch_merge_ln launch (16-bit o, fp32 lse, 16-bit out): per token,
    branch b contributes the E/r_b covered output columns and H/r_b LSE values."""
    E = H * D
    per_tok = sum(E / r * 2 + H / r * 4 for r in ratios) + E * 2
    return float(B * L * per_tok)


def attention_valid_flops_window(L: int, segs: Sequence[int], ratios: Sequence[int], H: int, D: int, lo: int,
                                 hi: int) -> float:
    """Valid attention FLOPs of the query rows whose sparse_to_dense slot lies in [lo, hi) (one
    sequence-parallel shard): each such (row, head) costs 4*D*c, c = real keys of its segment."""
    tot = 0.0
    p = np.arange(lo, hi, dtype=np.int64)
    for sl, r in zip(segs, ratios):
        s, nseg, m = branch_geometry(L, sl, r)
        hp = H + ((r - H % r) % r)
        hpg = hp // r
        g = m * r
        n = p // g
        j = (p % g) % r
        seg_len = np.minimum(L - n * s, s)                 # real tokens of the row's segment
        rem = seg_len - j
        c = np.where(rem > 0, -(-rem // r), 0)
        heads = np.clip(H - j * hpg, 0, hpg)
        real_q = (p % g) < seg_len                         # a zero-padded query row is not valid work
        tot += float((4.0 * D * c * heads * real_q).sum())
    return tot
