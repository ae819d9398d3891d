"""Host side of the packed key-row tail (no GPU): the new entries reject bad arguments before any launch
(fabricated, aligned device pointers), and runtime.packed_key_row_plan's tables against a numpy restatement."""
import ctypes

import numpy as np
import pytest

from test_attn_plan_host import D, E, H, QKV, RATIOS, ROWS, SEGS, _outs, i32, i64, lib, vp  # noqa: F401

LS, NB = [6001, 17, 1025], len(SEGS)


def _rows_plan(lib, qkv=QKV, Dh=D, bad_off=False, short=0):
    sched = ((i32 * NB)(*SEGS), (i32 * NB)(*RATIOS), NB)
    need = int(lib.gp_attn_rows_plan_varlen_bytes((i64 * 3)(*LS), 3, *sched))
    offs = [np.arange(sum(-(-L // min(sl, L)) * r for L in LS) + 1, dtype=np.int32) for sl, r in zip(SEGS, RATIOS)]
    for off in offs:
        off[3] -= 2 * bad_off
    return lib.gp_attn_rows_plan_varlen((i64 * 3)(*LS), 3, H, Dh, *sched, qkv, 3 * E,
                                        (vp * NB)(*[a.ctypes.data for a in offs]), (vp * NB)(*[ROWS] * NB), *_outs(NB),
                                        (ctypes.c_uint8 * need)(), need - short)


def _merge(lib, Hh=H, Dh=D, nbr=NB, plan_dev=QKV, rows=ROWS, out=QKV):
    need = int(lib.gp_varlen_plan_bytes(3, NB))
    plan, el = (ctypes.c_uint8 * need)(), (i64 * NB)()
    assert lib.gp_varlen_plan((i64 * 3)(*LS), 3, Hh, Dh, (i32 * NB)(*SEGS), (i32 * NB)(*RATIOS), nbr, QKV, 3 * Hh * Dh,
                              *_outs(NB), plan, need, el, el) == 0
    return lib.gp_branch_merge_ln_rows_varlen(plan, plan_dev, rows, 4, None, None, 1e-5, out, 0, None)


def _cls(lib, Dh=D, row_map=ROWS, map_off=ROWS + 4096, map_rows=100):
    return lib.gp_cls_attn_merge_ln_maps(QKV, QKV + 2 * E, QKV + 4 * E, 3 * E, ROWS, ROWS, 3, 6001, row_map, map_off,
                                         map_rows, H, Dh, (i32 * NB)(*SEGS), (i32 * NB)(*RATIOS), NB, 0.0, 1, 0, None,
                                         None, 1e-5, QKV, QKV, 0, None)


@pytest.mark.parametrize("call,kw,msg", [
    (_rows_plan, dict(qkv=None), b"null pointer"), (_rows_plan, dict(qkv=QKV + 8), b"16-byte aligned"),
    (_rows_plan, dict(Dh=64), b"head dim 64 unsupported"), (_rows_plan, dict(bad_off=True), b"bad list offsets (slide 0"),
    (_rows_plan, dict(short=16), b"plan buffer of"),
    (_merge, dict(Hh=12, Dh=64), b"H 12, D 64, 5 branches unsupported"), (_merge, dict(nbr=4), b"4 branches unsupported"),
    (_merge, dict(plan_dev=QKV + 8), b"null/misaligned plan"), (_merge, dict(rows=None), b"null pointer"),
    (_merge, dict(out=QKV + 8), b"out 16-byte aligned"),
    (_cls, dict(Dh=64), b"head dim 64 unsupported"), (_cls, dict(row_map=None), b"null/misaligned row_map"),
    (_cls, dict(map_off=ROWS + 4), b"null/misaligned row_map or map_off"), (_cls, dict(map_rows=0), b"map_rows = 0"),
    (_cls, dict(), b"workspace of 0 bytes")])
def test_new_entries_reject_before_launch(lib, call, kw, msg):
    assert _rows_plan(lib) == 0
    assert call(lib, **kw) == -1 and msg in lib.gp_last_error_string()


def test_packed_key_row_tables():
    """Product schedule: slides 0 and 2 list their S_i, the 600-token slide every token; 48.5 % in all."""
    from gigapath import runtime
    Ls, tok_off = [10000, 600, 8000], [0, 10000, 10600]
    p = runtime.packed_key_row_plan(Ls, SEGS, RATIOS)
    want_rows, want_map = [], []
    for L, t0 in zip(Ls, tok_off):
        keys = set()
        for sl, r in zip(SEGS, RATIOS):
            keys |= set(range(0, min(sl, L), r))
        S = sorted(keys) if len(keys) <= 0.5 * L else list(range(L))
        m = np.full(L, -1, dtype=np.int32)
        m[S] = np.arange(len(S))
        want_rows.append(np.array(S) + t0)
        want_map.append(m)
    n = [len(r) for r in want_rows]
    assert n[1] == 600 and sum(n) <= runtime.KEYROW_MAX_SHARE * sum(Ls)
    assert p["n"].tolist() == n and p["off"].tolist() == [0, n[0], n[0] + n[1]] and p["map_off"].tolist() == tok_off
    assert np.array_equal(p["rows"], np.concatenate(want_rows)) and p["rows"].dtype == np.int32
    assert np.array_equal(p["row_map"], np.concatenate(want_map))
    assert [int(off[-1]) for off, idx in p["groups"]] == [sum(n)] * NB == [idx.size for _, idx in p["groups"]]
