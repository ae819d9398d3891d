"""gp_dilated_attn_bwd2 without a GPU: the symbols, its argument errors (rejected on the host before any launch), its
workspace, and the switch that routes the training path to it."""
import pytest
import torch

from test_attn_bwd_host import FAKE
from test_dilated_bwd_host import SCHED_A, _i32, _tab, lib  # noqa: F401  (lib: the loaded library, a fixture)


def _ws(lib, L, D=48):
    return lib.gp_dilated_attn_bwd2_workspace_bytes(2, L, 16, D, _i32(SCHED_A[0]), _i32(SCHED_A[1]), len(SCHED_A[0]))


def test_symbols_are_exported_and_bound(lib):
    from gigapath import _hip
    for name in ("gp_dilated_attn_bwd2", "gp_dilated_attn_bwd2_workspace_bytes"):
        assert name in _hip.SIGNATURES and getattr(lib, name) is not None
    assert callable(_hip.dilated_attn_bwd2)


@pytest.mark.parametrize("kw,msg", [
    ({"D": 64}, b"head dim D = 64"),
    ({"D": 96}, b"head dim D = 96"),
    ({"pre": 0}, b"q_log2_prescaled must be 1"),
    ({"fmt": 2}, b"bad fmt 2"),
    ({"dq": None}, b"null pointer (dq)"),
    ({"dmerged": FAKE + 8}, b"misaligned pointer (dmerged)"),
    ({"short": 1}, b"workspace too small"),
], ids=lambda v: "-".join(v) if isinstance(v, dict) else None)
def test_argument_errors_are_rejected_on_the_host(lib, kw, msg):
    a = {**dict(D=48, pre=1, fmt=0, dq=FAKE, dmerged=FAKE, short=0), **kw}
    n, L, H = len(SCHED_A[0]), 200, 16
    assert lib.gp_dilated_attn_bwd2(FAKE, FAKE, FAKE, 3 * H * a["D"], 2, L, H, a["D"], _i32(SCHED_A[0]), _i32(SCHED_A[1]),
                                    n, _tab(n), _tab(n), a["dmerged"], 0.0, a["pre"], a["dq"], FAKE, FAKE,
                                    3 * H * a["D"], FAKE, _ws(lib, L) - a["short"], a["fmt"], None) == -1
    assert msg in lib.gp_last_error_string()


def test_workspace_is_monotone_in_L(lib):
    sizes = [_ws(lib, L) for L in (1, 5, 200, 257, 1500, 70001)]
    assert sizes[0] > 0 and sizes == sorted(sizes) and len(set(sizes)) == len(sizes)
    assert _ws(lib, 200, D=64) == 0 and _ws(lib, 0) == 0


def test_switch_reaches_every_dilated_attention():
    from gigapath import runtime, slide_encoder
    from gigapath.torchscale.component.dilated_attention import DilatedAttention
    model = slide_encoder.create_model("", "gigapath_slide_enc12l768d", 1536)
    attns = [m for m in model.modules() if isinstance(m, DilatedAttention)]
    assert len(attns) == 12 and all(runtime.attn_bwd2_enabled(m) == runtime.TRAIN_ATTN_BWD2 for m in attns)
    for flag in (True, False):
        model.enable_training(True, native_attn_bwd2=flag)
        assert all(runtime.attn_bwd2_enabled(m) == flag and m.native_dgrad is None for m in attns)
    model.enable_training(True, native_attn_bwd2=True)
    model.enable_training(True)                                 # None leaves it alone
    assert all(m.native_attn_bwd2 is True for m in attns)
