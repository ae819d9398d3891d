"""Packed (varlen) batches at D = 96, CPU side (no GPU): what runtime.varlen_covers admits, and the entries' host
checks on a plan built over fabricated pointers -- every rejection comes before any launch."""
import ctypes
import itertools

import torch

from test_attn_bwd_host import FAKE
from test_dilated_bwd_host import SCHED_A
from test_varlen_bwd_host import LS, _host, _i32, _i64, _tab, lib  # noqa: F401  (lib: the fixture)

H, D, E = 16, 96, 1536
BF16, F16, F16_VBF16 = 0, 1, 2                                      # GP_FMT_*


def test_varlen_covers_truth_table():
    from gigapath import runtime
    for d, act, grad in itertools.product((48, 64, 96), (torch.bfloat16, torch.float16), (False, True)):
        assert runtime.varlen_covers(d, act, grad=grad) is (d == 48 or (act == torch.bfloat16 and not grad)), (d, act, grad)


def test_entries_on_a_d96_plan(lib):  # noqa: F811
    nbytes = lib.gp_varlen_plan_bytes(len(LS), 5)
    host, o_el, l_el = _host(nbytes), _i64([0] * 5), _i64([0] * 5)
    assert lib.gp_varlen_plan(_i64(LS), len(LS), H, D, _i32(SCHED_A[0]), _i32(SCHED_A[1]), 5, FAKE, 3 * E, _tab(8),
                              _tab(8), host, nbytes, o_el, l_el) == 0
    err = lib.gp_last_error_string
    for fmt, pre in ((F16, 0), (F16_VBF16, 0), (BF16, 1)):
        assert lib.gp_dilated_attn_fwd_varlen(host, FAKE, pre, fmt, None) == -1, (fmt, pre)   # GP_EARG
        assert b"D = 96 needs bf16 and a q that is not pre-scaled" in err()
    # the merge gets past its shape check at 1536 / 96: the next check (a null output) is the one that fires
    assert lib.gp_branch_merge_ln_varlen(host, FAKE, None, None, ctypes.c_float(1e-5), None, BF16, None) == -1
    assert b"bad output / LN arguments" in err()
