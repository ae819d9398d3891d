"""The attention launch plans, pinned byte for byte (CPU only: gp_varlen_plan, gp_attn_rows_plan and
gp_attn_launch_params never touch the GPU).  The device pointers are fabricated, suitably aligned integers
that the planners only do arithmetic on; the plan buffer is zero-filled first, so its SHA-256 covers the
work tables (branch order, item counts, division magics, per-entry pointers) and the header.

The expected digests are those the library built from the commit BEFORE the attention source was split
into gp_attn.hip / gp_merge.hip / gp_sparsify.hip produced: a refactor of the planners' host code must
reproduce them; a deliberate change of a plan's layout has to re-record them."""
import ctypes
import hashlib

import pytest

import oracle as orc

CFG = orc.arch_config("gigapath_slide_enc12l768d")
SEGS, RATIOS = list(CFG["segment_length"]), list(CFG["dilated_ratio"])
H, D = 16, 48
E = H * D
QKV = 0x10000000                      # fabricated device addresses (never dereferenced), 16-byte aligned
ROWS = 0x30000000
O_BASE, LSE_BASE, STEP = 0x200000000, 0x600000000, 0x40000000

i32, i64, vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p


@pytest.fixture(scope="module")
def lib():
    from test_abi_and_api import _lib_path
    _lib_path()
    from gigapath import _hip
    return _hip.load_library()


def _sha(buf):
    return hashlib.sha256(bytes(buf)).hexdigest()


def _outs(nb):
    return ((vp * nb)(*[O_BASE + b * STEP for b in range(nb)]), (vp * nb)(*[LSE_BASE + b * STEP for b in range(nb)]))


def _varlen(lib, Ls, segs, ratios, plan_bytes=None, nbranch=None):
    """(rc, sha of the plan bytes, sha of o_elems | lse_elems) of gp_varlen_plan on fabricated pointers."""
    nb = len(segs) if nbranch is None else nbranch
    need = int(lib.gp_varlen_plan_bytes(len(Ls), len(segs)))
    assert need > 0 and need % 16 == 0
    plan = (ctypes.c_uint8 * need)()
    o_el, l_el = (i64 * len(segs))(), (i64 * len(segs))()
    o, lse = _outs(len(segs))
    rc = lib.gp_varlen_plan((i64 * len(Ls))(*Ls), len(Ls), H, D, (i32 * len(segs))(*segs), (i32 * len(ratios))(*ratios),
                            nb, QKV, 3 * E, o, lse, plan, need if plan_bytes is None else plan_bytes, o_el, l_el)
    return rc, _sha(plan), _sha(bytes(o_el) + bytes(l_el))


def _geometry(L, sl, r):
    s = min(sl, L)
    return -(-L // s), -(-s // r)      # nseg, m


def _rows(lib, B, L, segs, ratios, counts, plan_bytes=None, nbranch=None, flip=None):
    """(rc, sha of the plan bytes) of gp_attn_rows_plan; counts[b][n * r + j] listed rows of each (segment, phase)
    group of branch b.  flip = (branch, group): that group's end offset runs backwards."""
    nb = len(segs) if nbranch is None else nbranch
    offs = []
    for b, (sl, r) in enumerate(zip(segs, ratios)):
        nseg, m = _geometry(L, sl, r)
        assert len(counts[b]) == nseg * r and max(counts[b]) <= m
        off = [0]
        for c in counts[b]:
            off.append(off[-1] + c)
        if flip is not None and flip[0] == b:
            off[flip[1] + 1] = off[flip[1]] - 1
        offs.append((i32 * len(off))(*off))
    n = len(segs)
    need = int(lib.gp_attn_rows_plan_bytes(B, L, (i32 * n)(*segs), (i32 * n)(*ratios), n))
    assert need > 64
    plan = (ctypes.c_uint8 * need)()
    o, lse = _outs(n)
    rc = lib.gp_attn_rows_plan(QKV, QKV + 2 * E, QKV + 4 * E, 3 * E, B, L, H, D, (i32 * n)(*segs), (i32 * n)(*ratios), nb,
                               (vp * n)(*[ctypes.addressof(a) for a in offs]),
                               (vp * n)(*[ROWS + b * STEP for b in range(n)]), o, lse, plan,
                               need if plan_bytes is None else plan_bytes)
    return rc, _sha(plan)


def _cycle(pattern, n, shift=0):
    return [pattern[(k + shift) % len(pattern)] for k in range(n)]


# groups per branch at L = 4097 with the product schedule: 5, 2, 4, 8, 16 (m = 1024, 2049, 1025, 513, 257).
# Lists that are empty, of 1 row, of exactly one query block (256 rows at 8 waves x 32) and of one row more.
PATTERN = [0, 1, 256, 257, 0, 7]
COUNTS_4097 = [_cycle(PATTERN, n, b) for b, n in enumerate((5, 2, 4, 8, 16))]
# m = 512, 1024, 1024, 1024: the three equal branches come first, in their input order (a stable sort)
TIE_SEGS, TIE_RATIOS = [512, 2048, 1024, 4096], [1, 2, 1, 4]
COUNTS_TIE = [_cycle([3, 0, 256], n, b) for b, n in enumerate((9, 6, 5, 8))]

# Recorded from the parent commit's library (see the module docstring).
VARLEN_CASES = {
    "pack4": ([1, 31, 1025, 4097], SEGS, RATIOS,
              "f10e20c5d819aec9d78c4fd3bf49794bb0bda7135055644fdbdf7de84f51495d",
              "979081a4f3f06041377b51a728304632b738cb3b29fa08dff3db60d0602db0e6"),
    "single": ([600], SEGS, RATIOS,
               "fa862fccb664a185b23af13c64b75fc788ccd98e62ba286aa589e59ab95117fd",
               "5bcda16815105b8afaafa68ce418bbe9cecb65e1f6e15aa156c94c8fcc167c4a"),
    "two_branch": ([700, 3000, 5000], [1024, 4096], [1, 2],
                   "ebbfb280b1c89d78c356bd7834f47da35aa2facd7b916c72f8b03fde7e8adaef",
                   "8cf9822ea917706237d65043439ee2014ce24e62d37409f8bc52e9df3a3efbb8"),
}
ROWS_CASES = {
    "product_4097": (4097, SEGS, RATIOS, COUNTS_4097,
                     "1817baaeefe75eef8a0f6d774afa524942bd63cd829df301a18aecde4e030ef8"),
    "equal_m": (4097, TIE_SEGS, TIE_RATIOS, COUNTS_TIE,
                "623fd93793d46a54cc75bf31349853ac151f5e24321a781b938e447e22772adc"),
}


def test_launch_params(lib):
    p = (i32 * 4)()
    assert lib.gp_attn_launch_params(ctypes.cast(p, vp), 4) == 0
    assert list(p) == [256, 3, 3, 64]     # rows per 8-wave item, workgroups per CU, under-filled items per CU, key parts


@pytest.mark.parametrize("name", sorted(VARLEN_CASES))
def test_varlen_plan_bytes_are_pinned(lib, name):
    Ls, segs, ratios, want_plan, want_el = VARLEN_CASES[name]
    rc, plan, el = _varlen(lib, Ls, segs, ratios)
    assert rc == 0, lib.gp_last_error_string()
    assert (plan, el) == (want_plan, want_el)


@pytest.mark.parametrize("name", sorted(ROWS_CASES))
def test_rows_plan_bytes_are_pinned(lib, name):
    L, segs, ratios, counts, want = ROWS_CASES[name]
    rc, plan = _rows(lib, 2, L, segs, ratios, counts)
    assert rc == 0, lib.gp_last_error_string()
    assert plan == want


def test_plan_errors_still_fire(lib):
    Ls = [1, 31, 1025, 4097]
    need = int(lib.gp_varlen_plan_bytes(len(Ls), 5))
    assert _varlen(lib, Ls, SEGS, RATIOS, plan_bytes=need - 16)[0] == -1
    assert b"gp_varlen_plan: plan buffer" in lib.gp_last_error_string()
    assert _varlen(lib, Ls, SEGS, RATIOS, nbranch=0)[0] == -1
    assert b"gp_varlen_plan: nbranch must be 1..8" in lib.gp_last_error_string()
    assert lib.gp_varlen_plan_bytes(4, 0) == -1

    need = int(lib.gp_attn_rows_plan_bytes(2, 4097, (i32 * 5)(*SEGS), (i32 * 5)(*RATIOS), 5))
    assert _rows(lib, 2, 4097, SEGS, RATIOS, COUNTS_4097, plan_bytes=need - 1)[0] == -1
    assert b"gp_attn_rows_plan: plan buffer of" in lib.gp_last_error_string()
    assert _rows(lib, 2, 4097, SEGS, RATIOS, COUNTS_4097, nbranch=0)[0] == -1
    assert b"gp_attn_rows_plan: plan buffer of" in lib.gp_last_error_string()      # no size for no branches
    assert lib.gp_attn_rows_plan_bytes(2, 4097, (i32 * 5)(*SEGS), (i32 * 5)(*RATIOS), 0) == -1
    assert _rows(lib, 2, 4097, SEGS, RATIOS, COUNTS_4097, flip=(2, 1))[0] == -1
    assert b"gp_attn_rows_plan: bad list offsets (branch 2)" in lib.gp_last_error_string()
