"""The packed (varlen) dilated attention backward, CPU side (no GPU): gp_varlen_bwd_plan_bytes, gp_varlen_bwd_plan and
gp_dilated_attn_bwd_varlen are exported under ABI 13, reject every argument error on the host before any launch (fake
device pointers, as tests/test_dilated_bwd_host.py does), and size the workspace and the per-branch launches as a
numpy restatement of the geometry says.
"""
import ctypes

import numpy as np
import pytest

from test_attn_bwd_host import FAKE
from test_dilated_bwd_host import SCHED_A, SCHED_B

SCHED_ARCH = ([1024, 5792, 32768, 185363, 1048576], [1, 2, 4, 8, 16])      # gigapath_slide_enc12l768d
H, D, E = 16, 48, 768
LS = [200, 5, 31, 1, 333]


@pytest.fixture(scope="module")
def lib():
    from test_abi_and_api import _lib_path
    _lib_path()
    from gigapath import _hip
    return _hip.load_library()


def _i32(vals):
    return (ctypes.c_int32 * len(vals))(*vals)


def _i64(vals):
    return (ctypes.c_int64 * len(vals))(*vals)


def _tab(n, val=FAKE):
    return (ctypes.c_void_p * n)(*([val] * n))


def _host(nbytes):
    return (ctypes.c_uint64 * ((nbytes + 7) // 8))()


def _plan(lib, Ls=LS, H=H, D=D, segs=SCHED_A[0], ratios=SCHED_A[1], nbranch=None, qkv=FAKE, stride=None, o_in="tab",
          lse_in="tab", host="new", plan_bytes=None, ws_out="new"):
    """gp_varlen_bwd_plan with fake device pointers -> (rc, host buffer, workspace bytes)."""
    n = len(segs) if nbranch is None else nbranch
    need = lib.gp_varlen_bwd_plan_bytes(len(Ls) if Ls is not None else 1, max(1, min(n, 8)))
    buf = _host(need) if host == "new" else host
    ws = ctypes.c_int64(-1)
    segs, ratios = list(segs) + [1] * 8, list(ratios) + [1] * 8
    rc = lib.gp_varlen_bwd_plan(_i64(Ls) if Ls is not None else None, len(Ls) if Ls is not None else 1, H, D,
                                _i32(segs), _i32(ratios), n, qkv, 3 * H * D if stride is None else stride,
                                _tab(8) if o_in == "tab" else o_in, _tab(8) if lse_in == "tab" else lse_in, buf,
                                need if plan_bytes is None else plan_bytes,
                                ctypes.byref(ws) if ws_out == "new" else ws_out)
    return rc, buf, ws.value


def _launch(lib, host, dev=FAKE, dmerged=FAKE, dq=FAKE, dk=FAKE, dv=FAKE, ds=3 * E, ws=FAKE, ws_bytes=1 << 40, fmt=0):
    return lib.gp_dilated_attn_bwd_varlen(host, dev, dmerged, dq, dk, dv, ds, ws, ws_bytes, fmt, None)


def test_symbols_are_exported_under_abi_13(lib):
    from gigapath import _hip
    assert lib.gp_abi_version() == 13 == _hip.ABI_VERSION
    for name in ("gp_varlen_bwd_plan_bytes", "gp_varlen_bwd_plan", "gp_dilated_attn_bwd_varlen"):
        assert name in _hip.SIGNATURES
        assert getattr(lib, name) is not None


def test_plan_argument_errors_are_rejected_on_the_host(lib):
    err = lib.gp_last_error_string
    assert lib.gp_varlen_bwd_plan_bytes(0, 5) == -1 and lib.gp_varlen_bwd_plan_bytes(3, 0) == -1
    assert lib.gp_varlen_bwd_plan_bytes(3, 9) == -1 and lib.gp_varlen_bwd_plan_bytes(3, 5) > 0
    assert _plan(lib)[0] == 0
    assert _plan(lib, Ls=None)[0] == -1 and b"null pointer (L)" in err()
    assert _plan(lib, ws_out=None)[0] == -1 and b"null pointer (workspace_bytes)" in err()
    assert _plan(lib, D=64)[0] == -1 and b"head dim 64" in err()
    assert _plan(lib, H=0)[0] == -1 and b"bad H 0" in err()
    assert _plan(lib, nbranch=0)[0] == -1 and b"nbranch must be 1..8" in err()
    assert _plan(lib, nbranch=9)[0] == -1 and b"nbranch must be 1..8" in err()
    assert _plan(lib, ratios=[1, 2, 0, 8, 16])[0] == -1 and b"branch 2: bad seg_len 90 / ratio 0" in err()
    assert _plan(lib, segs=[32, 60, 90, 0, 1000])[0] == -1 and b"branch 3: bad seg_len 0" in err()
    assert _plan(lib, Ls=[5, 0, 7])[0] == -1 and b"slide 1 has L = 0" in err()
    assert _plan(lib, stride=3 * E - 8)[0] == -1 and b"qkv_row_stride 2296 below 3*H*D = 2304" in err()
    assert _plan(lib, stride=3 * E + 4)[0] == -1 and b"not a multiple of 8" in err()
    # T >= 2^31, and a branch whose item count passes 2^31 while T does not (H = 4096, one-token segments)
    assert _plan(lib, Ls=[1 << 30, 1 << 30])[0] == -1 and b"packed tokens exceed 2^31 - 1" in err()
    assert _plan(lib, Ls=[1 << 20], H=4096, segs=[1], ratios=[1])[0] == -1 and b"work items exceed one launch" in err()
    # the pointers the table stores
    assert _plan(lib, qkv=None)[0] == -1 and b"null pointer (qkv)" in err()
    assert _plan(lib, qkv=FAKE + 8)[0] == -1 and b"misaligned pointer (qkv)" in err()
    assert _plan(lib, o_in=None)[0] == -1 and b"null pointer (o_in)" in err()
    assert _plan(lib, lse_in=None)[0] == -1 and b"null pointer (lse_in)" in err()
    assert _plan(lib, o_in=_tab(8, None))[0] == -1 and b"null pointer (o_in / lse_in [0])" in err()
    assert _plan(lib, o_in=_tab(8, FAKE + 8))[0] == -1 and b"misaligned pointer (o_in / lse_in [0])" in err()
    assert _plan(lib, lse_in=_tab(8, FAKE + 2))[0] == -1 and b"misaligned pointer (o_in / lse_in [0])" in err()
    assert _plan(lib, plan_bytes=64)[0] == -1 and b"plan buffer 64 <" in err()


def test_sizing_call_needs_no_pointers(lib):
    rc, _, ws = _plan(lib, qkv=None, o_in=None, lse_in=None, host=None, plan_bytes=0)
    assert rc == 0 and ws == _plan(lib)[2] > 0


def test_launch_argument_errors_are_rejected_on_the_host(lib):
    err = lib.gp_last_error_string
    rc, host, need = _plan(lib)
    assert rc == 0
    assert _launch(lib, host, fmt=7) == -1 and b"bad fmt 7" in err()
    assert _launch(lib, host, fmt=2) == -1 and b"bad fmt 2" in err()                  # GP_FMT_F16_VBF16
    assert _launch(lib, None) == -1 and b"null pointer (plan_host)" in err()
    assert _launch(lib, host, dev=None) == -1 and b"null pointer (plan_dev)" in err()
    assert _launch(lib, host, dev=FAKE + 8) == -1 and b"misaligned pointer (plan_host 8 bytes / plan_dev" in err()
    for nm in ("dmerged", "dq", "dk", "dv"):
        assert _launch(lib, host, **{nm: None}) == -1 and b"null pointer (%s)" % nm.encode() in err()
        assert _launch(lib, host, **{nm: FAKE + 8}) == -1 and b"misaligned pointer (%s)" % nm.encode() in err()
    assert _launch(lib, host, ds=760) == -1 and b"d_row_stride 760 below H*D = 768" in err()
    assert _launch(lib, host, ds=772) == -1 and b"not a multiple of 8" in err()
    assert _launch(lib, host, ws_bytes=need - 1) == -1 and b"workspace too small" in err()
    assert _launch(lib, host, ws=None) == -1 and b"workspace too small" in err()
    assert _launch(lib, host, ws=FAKE + 4, ws_bytes=need) == -1 and b"misaligned workspace" in err()
    # not a backward plan: zeros, and the forward's plan of the same pack
    assert _launch(lib, _host(4096)) == -1 and b"not a gp_varlen_bwd_plan buffer" in err()
    fwd_bytes = lib.gp_varlen_plan_bytes(len(LS), 5)
    fwd = _host(fwd_bytes)
    o_el, l_el = _i64([0] * 5), _i64([0] * 5)
    assert lib.gp_varlen_plan(_i64(LS), len(LS), H, D, _i32(SCHED_A[0]), _i32(SCHED_A[1]), 5, FAKE, 3 * E, _tab(8),
                              _tab(8), fwd, fwd_bytes, o_el, l_el) == 0
    assert _launch(lib, fwd) == -1 and b"not a gp_varlen_bwd_plan buffer" in err()


def _restate(Ls, segs, ratios):
    """(workspace bytes, items per branch, o elements per branch, lse elements per branch) in numpy."""
    Ls = np.asarray(Ls, dtype=np.int64)
    up = lambda n: (n + 255) // 256 * 256
    total, items, o_el, l_el = 0, [], [], []
    for sl, r in zip(segs, ratios):
        s = np.minimum(sl, Ls)
        nseg, m = -(-Ls // s), -(-s // r)
        items.append(int((nseg * H * -(-m // 128)).sum()))
        rows = int((nseg * m * H).sum())
        o_el.append(rows * D)
        l_el.append(rows)
        total += up(rows * D * 2) + up(rows * 4)
    total += 3 * up(int(Ls.sum()) * E * 4)
    return total, items, o_el, l_el


@pytest.mark.parametrize("Ls,sched", [([1, 2, 17, 257, 1500], SCHED_A), ([1, 2, 17, 257, 1500], SCHED_B),
                                      ([1025, 2897, 700], SCHED_ARCH)], ids=["A", "B", "arch"])
def test_workspace_and_item_counts_match_the_restatement(lib, Ls, sched):
    from gigapath import _hip
    segs, ratios = sched
    rc, host, ws = _plan(lib, Ls=Ls, segs=segs, ratios=ratios)
    assert rc == 0
    want_ws, want_items, want_o, want_l = _restate(Ls, segs, ratios)
    hdr = _hip.VarlenBwdHdr.from_buffer(host)
    assert (hdr.nslide, hdr.nbranch, hdr.H, hdr.D, hdr.T) == (len(Ls), len(segs), H, D, sum(Ls))
    assert list(hdr.items)[:len(segs)] == want_items
    assert ws == want_ws
    # the regions are the forward plan's: the backward reads o / lse and writes dout / delta in those layouts
    fwd = _hip.VarlenPlan(Ls, H, D, segs, ratios)
    assert fwd.o_elems == want_o and fwd.lse_elems == want_l
    bwd = _hip.VarlenBwdPlan(Ls, H, D, segs, ratios)
    assert bwd.workspace_bytes == want_ws and bwd.nbytes == lib.gp_varlen_bwd_plan_bytes(len(Ls), len(segs))
