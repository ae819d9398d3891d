"""The key-row tail's host planner (gigapath.runtime.key_row_plan) against a brute-force
construction from the oracle's index maps: the rows S are the tokens gather_index (dense_to_sparse) feeds to
token 0's query, the per-group lists are the sparse rows scatter_index (sparse_to_dense) reads back for the
tokens of S.  No GPU, no library."""
import numpy as np
import pytest

import oracle as orc
from gigapath import runtime

CFG = orc.arch_config("gigapath_slide_enc12l768d")
PRODUCT = (tuple(CFG["segment_length"]), tuple(CFG["dilated_ratio"]))
SCALED = ((64, 362, 2048), (1, 2, 4))
H = 16
CASES = [(PRODUCT, 1025), (PRODUCT, 4098), (PRODUCT, 6001), (PRODUCT, 10001), (PRODUCT, 70001), (SCALED, 2500)]
COUNTS = {10001: 4461, 70001: 14807}

_PLANS = {}


def _plan(sched, L):
    key = (sched, L)
    if key not in _PLANS:
        _PLANS[key] = runtime.key_row_plan(L, *sched)
    return _PLANS[key]


def _brute_rows(sched, L):
    """Tokens that are a key of token 0 (sparse row 0 of segment 0, the heads of group 0) in some branch."""
    keys = set()
    for sl, r in zip(*sched):
        hpg = orc.branch_geometry(L, sl, r, H)["hpg"]
        tok = orc.gather_index(L, sl, r, H)[0, :min(hpg, H)]
        keys.update(int(t) for t in tok[tok >= 0])
    return np.array(sorted(keys), dtype=np.int64)


@pytest.mark.parametrize("sched,L", CASES)
def test_rows_are_token_zeros_keys(sched, L):
    rows, row_map, _ = _plan(sched, L)
    want = _brute_rows(sched, L)
    assert rows.dtype == np.int32 and row_map.dtype == np.int32
    assert np.array_equal(rows, want)
    if sched is PRODUCT and L in COUNTS:
        assert rows.size == COUNTS[L]
    if L <= 1025:
        assert rows.size == L                      # one segment of branch 0: every row


@pytest.mark.parametrize("sched,L", CASES)
def test_row_map_inverts_the_list(sched, L):
    rows, row_map, _ = _plan(sched, L)
    assert row_map.shape == (L,)
    assert np.array_equal(row_map[rows], np.arange(rows.size))
    out = np.ones(L, dtype=bool)
    out[rows] = False
    assert (row_map[out] == -1).all()
    assert rows[0] == 0                            # the CLS token is compact row 0


@pytest.mark.parametrize("sched,L", CASES)
def test_group_lists_match_scatter_index(sched, L):
    rows, _, groups = _plan(sched, L)
    assert len(groups) == len(sched[0])
    for (sl, r), (off, idx) in zip(zip(*sched), groups):
        geo = orc.branch_geometry(L, sl, r, H)
        nseg, m, hpg = geo["nseg"], geo["m"], geo["hpg"]
        assert off.dtype == np.int32 and idx.dtype == np.int32
        assert off.shape == (nseg * r + 1,) and off[0] == 0 and off[-1] == idx.size
        assert (np.diff(off) >= 0).all()
        # brute force: the (segment, sparse row) sparse_to_dense reads for token p and the first head of each group
        n_idx, i_idx = orc.scatter_index(L, sl, r, H)
        want = {}
        for j in range(r):
            h = j * hpg
            if h >= H:
                continue
            col_n, col_i = n_idx[rows, h], i_idx[rows, h]
            cov = col_n >= 0
            for n, i in zip(col_n[cov], col_i[cov]):
                want.setdefault((int(n), j), []).append(int(i))
        listed = set()
        for n in range(nseg):
            for j in range(r):
                got = idx[off[n * r + j]:off[n * r + j + 1]]
                assert (np.diff(got) > 0).all() and (got >= 0).all() and (got < m).all()
                if j * hpg < H:
                    assert got.tolist() == sorted(want.get((n, j), [])), (sl, r, n, j)
                # every listed row is a real query row of its segment: token n s + i r + j exists
                tok = n * geo["s"] + got.astype(np.int64) * r + j
                assert (tok < min(L, (n + 1) * geo["s"])).all()
                listed.update(tok.tolist())
        # the union over the groups of a branch is exactly S: every token is listed once per branch
        assert off[-1] == rows.size
        assert listed == set(rows.tolist())


def test_engagement_threshold():
    """|S| <= L / 2 from L = 7,842 on with the product schedule; never at the lengths of the bit-identity tests."""
    segs, ratios = PRODUCT
    share = lambda L: runtime.key_row_plan(L, segs, ratios)[0].size / L   # noqa: E731
    assert share(7841) > runtime.KEYROW_MAX_SHARE >= share(7842)
    for L in (2, 601, 1025, 4098):
        assert share(L) > runtime.KEYROW_MAX_SHARE
    assert share(70001) < 0.22 and share(256001) < 0.14
