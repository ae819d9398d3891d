"""The packed attention backward at D = 64 (gp_varlen_bwd2_plan_bytes, gp_varlen_bwd2_plan,
gp_dilated_attn_bwd2_varlen), CPU side: exported and bound under ABI 13, every argument error rejected on the host before
any launch (fake device pointers), a sizing call that needs no pointers, and the switch that admits D = 64 training."""
import ctypes

import pytest
import torch

from test_attn_bwd_host import FAKE
from test_dilated_bwd_host import SCHED_A
from test_varlen_bwd_host import _host, _i32, _i64, _tab, lib  # noqa: F401  (lib: the loaded library, a fixture)

H, D, E = 16, 64, 1024
LS = [200, 5, 31, 1, 333]


def _plan(lib, Ls=LS, D=D, sizing=False):
    need = lib.gp_varlen_bwd2_plan_bytes(len(Ls), 5)
    buf, ws = _host(need), ctypes.c_int64(-1)
    ptrs = (None, 3 * H * D, None, None, None, 0) if sizing else (FAKE, 3 * H * D, _tab(8), _tab(8), buf, need)
    rc = lib.gp_varlen_bwd2_plan(_i64(Ls), len(Ls), H, D, _i32(SCHED_A[0]), _i32(SCHED_A[1]), 5, *ptrs, ctypes.byref(ws))
    return rc, buf, ws.value


def _launch(lib, host, ws_bytes=1 << 40, prescaled=1, fmt=0):
    return lib.gp_dilated_attn_bwd2_varlen(host, FAKE, FAKE, FAKE, FAKE, FAKE, 3 * E, FAKE, ws_bytes, prescaled, fmt, None)


def test_symbols_are_exported_and_bound(lib):
    from gigapath import _hip
    assert lib.gp_abi_version() == 13 == _hip.ABI_VERSION
    for name in ("gp_varlen_bwd2_plan_bytes", "gp_varlen_bwd2_plan", "gp_dilated_attn_bwd2_varlen"):
        assert name in _hip.SIGNATURES and getattr(lib, name) is not None
    assert callable(_hip.dilated_attn_bwd2_varlen) and issubclass(_hip.VarlenBwd2Plan, _hip.VarlenBwdPlan)


def test_argument_errors_and_the_sizing_call(lib):
    from gigapath import _hip
    err = lib.gp_last_error_string
    rc, host, need = _plan(lib)
    assert rc == 0 and need > 0
    assert _plan(lib, sizing=True)[::2] == (0, need)                       # no pointers needed
    hdr = _hip.VarlenBwdHdr.from_buffer(host)
    assert (hdr.nslide, hdr.nbranch, hdr.H, hdr.D, hdr.T) == (5, 5, H, D, sum(LS))
    # 256-row own blocks: every (slide, segment, head) of branch 0 (segments of 32) is one work item
    assert hdr.items[0] == H * sum(-(-L // min(SCHED_A[0][0], L)) for L in LS)
    for d in (48, 96):
        assert _plan(lib, D=d)[0] == -1 and b"D = %d unsupported (D = 64 only)" % d in err()
    assert _plan(lib, Ls=[200, 0, 31])[0] == -1 and b"slide 1 has L = 0" in err()
    assert _launch(lib, host, fmt=1) == -1 and b"bad fmt 1 (GP_FMT_BF16 only)" in err()          # fp16
    assert _launch(lib, host, prescaled=0) == -1 and b"q_log2_prescaled must be 1" in err()      # an unscaled q
    assert _launch(lib, host, ws_bytes=need - 1) == -1 and b"workspace too small" in err()
    assert _launch(lib, _host(4096)) == -1 and b"not a gp_varlen_bwd2_plan buffer" in err()
    hdr.D = 48
    assert _launch(lib, host) == -1 and b"corrupt plan header" in err()


def test_varlen_covers_admits_d64_training_with_the_switch():
    from gigapath import runtime
    bf, fp = torch.bfloat16, torch.float16
    assert runtime.varlen_covers(64, bf, True, bwd2=True) is True
    assert runtime.varlen_covers(64, bf, True, bwd2=False) is False
    assert runtime.varlen_covers(64, fp, True, bwd2=True) is False
    assert runtime.varlen_covers(96, bf, True, bwd2=True) is False
    qkv = torch.zeros(8, 3 * E, dtype=fp)
    with pytest.raises(ValueError, match="cover D = 48"):
        runtime.dilated_attention_grad_varlen(qkv, [8], H, D, *SCHED_A, bwd2=True)
