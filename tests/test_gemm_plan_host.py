"""The GEMM tile planner (csrc/gp_gemm_impl.h: make_plan, through gp_gemm_workspace_bytes) against its pure
Python restatement in tests/gemm_plan.py -- host only: without a device the library plans for 256 CUs
(device_cus()'s fallback).  This pins the planner and keeps the helper the GPU tests choose their row counts
with honest."""
import pytest

import gemm_plan

ARCH_E = (768, 1024, 1536)     # the three registered archs (slide_encoder.py); F = 4E, patch in_chans 1536


def _cus():
    """The CU count the library plans for: the device's when one is visible, else device_cus()'s fallback."""
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256


G = _cus()


def _arch_shapes():
    """(N, K) of every GEMM of the three archs: QKV, out-proj, fc1, fc2, patch embed."""
    out = []
    for E in ARCH_E:
        out += [(3 * E, E), (E, E), (4 * E, E), (E, 4 * E), (E, 1536)]
    return sorted(set(out))


@pytest.fixture(scope="module")
def lib():
    from test_abi_and_api import _lib_path
    _lib_path()
    from gigapath import _hip
    return _hip.load_library()


def test_fallback_plans_for_256_cus(lib):
    if G != 256:
        return                                           # (a device of another size: the sweep below covers it)
    ws = lib.gp_gemm_workspace_bytes
    assert ws(65537, 256, 768) == 2 * 256 * 256 * 4      # 257 tiles: rem 1, S = 2
    assert ws(65537, 256, 3072) == 4 * 256 * 256 * 4     # S = 4
    assert ws(65536, 256, 768) == 0                      # exactly one round
    assert ws(98304, 256, 768) == 128 * 2 * 256 * 256 * 4    # rem 128 = G / 2: the last split remainder
    assert ws(98305, 256, 768) == 0                      # rem 129
    assert ws(81920, 256, 3072) == 64 * 4 * 256 * 256 * 4    # rem 64 = G / 4
    assert ws(81921, 256, 3072) == 0
    assert ws(14807, 2304, 768) == 10 * 2 * 256 * 256 * 4    # the 70k slide's key-row QKV: 522 tiles
    assert ws(70001, 2304, 768) == 0                     # 2466 tiles, rem 162: unsplit


@pytest.mark.parametrize("N,K", _arch_shapes())
def test_workspace_bytes_match_the_python_plan(lib, N, K):
    ws = lib.gp_gemm_workspace_bytes
    tn = N // 256
    split = 0
    for mb in range(1, 1101):
        for M in ((mb - 1) * 256 + 1, mb * 256):         # both ends of the row block
            p = gemm_plan.plan(M, N, K, G)
            assert ws(M, N, K) == p.ws_bytes, (M, N, K, p)
            tiles = mb * tn
            assert p.n_dp + p.rem == tiles and p.ws_bytes == p.rem * p.S * 256 * 256 * 4
            if p.S > 1:
                split += 1
                assert p.S == (2 if K == 768 else 4) and tiles > G and p.n_dp % G == 0
                assert 0 < p.rem <= G // p.S and p.rem * 2 <= G
            else:
                assert p.rem == 0 and p.n_dp == tiles
    assert split > 0


def test_rows_for_lands_on_the_requested_remainder():
    for N, K in _arch_shapes():
        tn = N // 256
        for g in (256, 304, 64):                         # (other CU counts: the helper is device-independent)
            for rem in (0, 1, 5, 10, gemm_plan.max_split_rem(K, g), gemm_plan.max_split_rem(K, g) + 1):
                try:
                    M = gemm_plan.rows_for(N, K, g, rem)
                except ValueError:
                    # no row count reaches it: rem is not a multiple of gcd(N / 256, G)
                    import math
                    assert rem % math.gcd(tn, g) != 0
                    continue
                tiles = gemm_plan.tiles_of(M, N)
                assert tiles > g and tiles % g == rem and M % 256 == 113
                p = gemm_plan.plan(M, N, K, g)
                assert (p.rem == rem and p.S > 1) if 0 < rem <= gemm_plan.max_split_rem(K, g) else p.S == 1
                # the smallest such M: no fewer row blocks have more than G tiles and this remainder
                assert not any(j * tn > g and (j * tn) % g == rem for j in range(1, tiles // tn))
    with pytest.raises(ValueError):
        gemm_plan.rows_for(2304, 768, 256, 5, partial=0)
    with pytest.raises(ValueError):
        gemm_plan.rows_for(1024, 1024, 256, 3)            # 4 tiles per row block: multiples of 4 only


def test_helper_picks_match_the_issue_figures():
    # on 256 CUs: the QKV split tail's smallest remainder, and the smallest multi-round split plans
    assert gemm_plan.rows_for(2304, 768, 256, 10) <= 14807
    M, rem = gemm_plan.smallest_split_rows(2304, 768, 256)
    assert rem == 5 and 7000 < M < 7500
    assert 16000 < gemm_plan.smallest_split_rows(1024, 1024, 256)[0] < 17000
    assert 10500 < gemm_plan.smallest_split_rows(1536, 1536, 256)[0] < 11500
    assert 3500 < gemm_plan.smallest_split_rows(4608, 1536, 256)[0] < 4000
    M, rem = gemm_plan.panel_split_rows(768, 768, 256, mixed=True)
    assert gemm_plan.plan(M, 768, 768, 256).n_dp % 3 != 0 and M <= 25613
    assert gemm_plan.panel_split_rows(1536, 1536, 256, mixed=True) == (10865, 2)
    assert gemm_plan.panel_split_rows(1536, 6144, 256, mixed=False) == (32881, 6)
    assert gemm_plan.panel_split_rows(1024, 4096, 256, mixed=False) == (16497, 4)
    with pytest.raises(ValueError):
        gemm_plan.panel_split_rows(1024, 1024, 256, mixed=True)       # 256 CUs, 4 tiles per panel: never mixed
