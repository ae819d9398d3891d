"""The persistent GEMM's tile plan (csrc/gp_gemm_impl.h: make_plan) restated in pure Python, and the row
counts that put a launch on a chosen edge of it.  A helper for the tests (imported like sp_emulator), pinned
to the library by test_gemm_plan_host.py.

    tiles = ceil(M / 256) * (N / 256)        256 x 256 output tiles, row-panel major
    G     = min(tiles, CUs)                  one persistent workgroup per CU
    rem   = tiles % G                        tiles of the last, partial round
    split iff tiles > G, 0 < rem, rem * S <= G and rem * 2 <= G, with S = 2 for K = 768 and 4 otherwise:
          the tail round's rem tiles are cut S ways in K (rem * S workgroups), the fp32 partials go to the
          workspace (rem * S * 256 * 256 * 4 bytes) and a reduce kernel sums them and runs the epilogue.
"""
from collections import namedtuple

BM = BN = 256
Plan = namedtuple("Plan", "S n_dp rem ws_bytes")


def tiles_of(M, N):
    return -(-M // BM) * (N // BN)


def split_factor(K):
    return 2 if K == 768 else 4


def plan(M, N, K, G, allow_split=True):
    """(S, n_dp, rem, ws_bytes) of an M x N x K launch on a device with G CUs.  Unsplit plans (one tile after
    another, every tile data-parallel) are (1, tiles, 0, 0).  allow_split=False: the plan of a launch without
    a workspace, and of the GELU epilogues, which never split."""
    tiles = tiles_of(M, N)
    g = min(tiles, G)
    S = split_factor(K)
    rem = tiles % g
    if allow_split and tiles > g and 0 < rem and rem * S <= g and rem * 2 <= g:
        return Plan(S, tiles - rem, rem, rem * S * BM * BN * 4)
    return Plan(1, tiles, 0, 0)


def max_split_rem(K, G):
    """The largest tail the plan still splits: G/2 for S = 2, G/4 for S = 4."""
    return G // max(split_factor(K), 2)


def rows_for(N, K, G, rem, partial=113):
    """The smallest M with more than G tiles, tiles % G == rem, and `partial` rows (1..256) in its last row
    block -- so the tail round holds the partial-M tiles.  ValueError if no row count gives that remainder
    (N / 256 and G share a factor that rem lacks).  K does not enter (the remainder is the plan's whether or not
    it splits); it is taken so that call sites read like plan()."""
    if not (0 <= rem < G and 1 <= partial <= BM and N % BN == 0 and N > 0):
        raise ValueError("rows_for: bad arguments N=%d G=%d rem=%d partial=%d" % (N, G, rem, partial))
    tn = N // BN
    first = G // tn + 1                       # the first row-block count with more than G tiles
    for mb in range(first, first + G + 1):    # mb * tn mod G has a period of at most G
        if (mb * tn) % G == rem:
            M = (mb - 1) * BM + partial
            assert tiles_of(M, N) == mb * tn > G
            return M
    raise ValueError("rows_for: no M gives %d tail tiles for N=%d on %d CUs" % (rem, N, G))


def smallest_split_rows(N, K, G, partial=113):
    """(M, rem) of the smallest multi-round plan that splits, its last row block partial."""
    best = None
    for rem in range(1, max_split_rem(K, G) + 1):
        try:
            M = rows_for(N, K, G, rem, partial)
        except ValueError:
            continue
        if best is None or M < best[0]:
            best = (M, rem)
    if best is None:
        raise ValueError("no split plan for N=%d K=%d on %d CUs" % (N, K, G))
    assert plan(best[0], N, K, G).rem == best[1]
    return best


def panel_split_rows(N, K, G, mixed, partial=113):
    """(M, rem) of the smallest split plan whose first tail row panel is part data-parallel, part split (mixed:
    n_dp is not a multiple of N / 256, as with 25,613 rows for N = 768 on 256 CUs) or whose tail panels are all
    entirely split (not mixed).  ValueError if this N has no such plan on G CUs."""
    tn = N // BN
    best = None
    for rounds in range(1, tn + 1):           # n_dp = rounds * G: its residue mod tn repeats after tn rounds
        for rem in range(1, max_split_rem(K, G) + 1):
            tiles = rounds * G + rem
            if tiles % tn != 0 or ((rounds * G) % tn != 0) != bool(mixed):
                continue
            M = (tiles // tn - 1) * BM + partial
            if best is None or M < best[0]:
                best = (M, rem)
            break
    if best is None:
        raise ValueError("no %s split plan for N=%d K=%d on %d CUs" % ("mixed-panel" if mixed else "whole-panel", N,
                                                                       K, G))
    p = plan(best[0], N, K, G)
    assert p.rem == best[1] and (p.n_dp % tn != 0) == bool(mixed)
    return best
