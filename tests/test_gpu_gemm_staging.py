"""The ping-pong GEMM's A staging: a wave issues pp_na(T) = (4 T + 7) / 8 LDS-DMAs per A sub-tile (one for the 8-piece
sub-tiles of the 128-row tile and of the 160-row tile's second half) and every counted vmcnt is derived from those counts
(cbas_amd/csrc/gemm_f16_8ph.hip, file header).  A piece that is not staged, is staged to the wrong LDS rows, or is read
before it has landed changes rows of the result, so every case here is held to

  - the float64 reference and bound of the GEMM edge tests (test_gpu_kernel_reference.check_gemm: every element, canaries),
  - the bytes of a kernel this staging is no part of, on the same operands: the 128 x 128 kernel of gemm_f16.hip (fp16
    operands), the 128 x 128 split kernels of vit_f32.hip (precision 4), and for MX-fp8 operands - which only the ping-pong
    kernel takes - its 256-row tile, whose sub-tiles have all 16 pieces (same MFMAs in the same k order: bit-identical).

Shapes are the smallest at which a count or a piece can be wrong: K of two K-tiles (prologue and drain with no steady state
between them) and of twelve; one and two column tiles; M of one tile, and of one tile + 8 rows (a second tile of clamped
rows); one non-zero row of A in each 8-row piece in turn; more tiles than workgroup slots (the next tile's first K-tile is
staged under the epilogue with the new counts); a planner launch with a 128-row tail behind 256-row tiles (kind switch)."""
import numpy as np
import pytest

from oracle import kernel_ref as R
from test_gpu_fp8 import _dequant, _gemm_f8
from test_gpu_kernel_reference import check_gemm, gemm_reference, gemm_run, make_gemm, out_buffer

pytestmark = pytest.mark.gpu

PP_TILE = {128: 16, 160: 15, 192: 14, 256: 13}      # kernels.h GEMM_TILE_PP_*; 17 = the planner, 1 = gemm_f16.hip 128 x 128


def run_bytes(arith, epi, d, tile, **kw):
    out = gemm_run(arith, epi, d["A"], d["W"], d["bias"], M=d["M"], out=out_buffer(arith, epi, d), tile=tile, lam=d.get("lam"),
                   **kw)
    return out.view(np.uint8)


def check_fp16(epi, d, tile, label):
    """float64 bound + canaries, then the bytes of the 128 x 128 kernel."""
    out = check_gemm(0, epi, d, label, tile=tile)[1]
    assert np.array_equal(out.view(np.uint8), run_bytes(0, epi, d, 1)), label


@pytest.mark.parametrize("K", [128, 768])
@pytest.mark.parametrize("bm", [128, 160, 192, 256])
def test_forced_tiles_one_tile_and_one_tile_plus_8_rows(bm, K):
    rng = np.random.default_rng(1000 * bm + K)
    for N in (256, 512):
        for M in (bm, bm + 8):
            d = make_gemm(rng, R.EPI_RESID, M, N, K)
            check_fp16(R.EPI_RESID, d, PP_TILE[bm], f"pp {bm} M {M} N {N} K {K}")


@pytest.mark.parametrize("bm", [128, 160])
def test_single_nonzero_row_of_A_in_each_piece_in_turn(bm):
    """Only the piece holding the row contributes: a dropped piece leaves the row's accumulators at whatever the LDS held
    (the previous launch's zeros), a piece staged to the wrong rows moves the products to another row."""
    rng = np.random.default_rng(bm)
    N, K = 256, 128
    d = make_gemm(rng, R.EPI_RESID, bm, N, K, M_alloc=bm)
    rows = rng.standard_normal((bm // 8, K)).astype(np.float32)
    for piece in range(bm // 8):
        row = 8 * piece + (3 * piece + 1) % 8
        d["A"][:] = 0.0
        d["A"][row] = rows[piece]
        got = check_gemm(0, R.EPI_RESID, d, f"pp {bm} piece {piece} row {row}", tile=PP_TILE[bm])[0]
        idle = d["x0"].astype(np.float64) + d["lam"].astype(np.float64) * d["bias"].astype(np.float64)   # rows with a zero accumulator
        moved = np.abs(got - idle).max(axis=1) > 1e-3
        assert moved[row] and moved.sum() == 1, (bm, piece, np.nonzero(moved)[0])


@pytest.mark.parametrize("bm", [128, 160])
def test_persistent_walk_of_the_small_tiles(bm):
    """86 row panels x 3 column tiles = 258 tiles on at most 256 workgroups: at least two workgroups run a second tile,
    whose K-tile 0 was staged under the first one's epilogue."""
    rng = np.random.default_rng(86 + bm)
    d = make_gemm(rng, R.EPI_RESID, bm * 86, 768, 128)
    check_fp16(R.EPI_RESID, d, PP_TILE[bm], f"pp {bm} persistent M {bm * 86} N 768 K 128")


def test_planner_launch_with_a_128_row_tail():
    """gemm_f16_8ph_kernel<.., 4, 4, 1, ..>: 256-row tiles, then 128-row tiles from the same workgroups (the kind switch).
    The shape is the headline's own `up` problem at K = 128, for which pp_plan returns 37 main panels on 256 compute units
    (rows from 9 472 on are the tail).  A tail needs between two and three rounds of tiles: restating pp_plan on the host,
    every M x N it gives a tail has at least 37.7 M outputs (12 296 x 3 072 the smallest), so no smaller shape covers the
    switch, and the float64 reference of that many elements takes several seconds.  Every element, canaries included, is
    therefore held to the bytes of the 128 x 128 kernel, and the float64 bound to every tail row, the 256-row panel in front
    of the switch and the first panel."""
    M, N, K, row_t = 12864, 3072, 128, 37 * 256
    rng = np.random.default_rng(M + N)
    d = make_gemm(rng, R.EPI_RESID, M, N, K)
    out = gemm_run(0, R.EPI_RESID, d["A"], d["W"], d["bias"], M=M, out=out_buffer(0, R.EPI_RESID, d), tile=17, lam=d["lam"])
    assert np.array_equal(out.view(np.uint8), run_bytes(0, R.EPI_RESID, d, 1))
    rows = np.r_[0:256, row_t - 256:M]
    y, Ey, _ = gemm_reference(0, R.EPI_RESID, dict(d, A=d["A"][rows], M=len(rows), x0=d["x0"][rows]))
    r = R.ratio(out[rows, :N].astype(np.float64), y, Ey)
    print(f"  pp planner main + tail M {M} N {N} K {K}: max err / bound = {r:.3g} on {len(rows)} rows")
    assert r <= 1.0, r


@pytest.mark.parametrize("bm", [128, 160])
def test_mx_fp8_form_of_the_small_tiles(bm):
    """The scale DMA rides with A-sub1 and is part of the derived counts.  K = 256 is the form's two K-tiles."""
    from oracle import mx_oracle as MX  # noqa: F401  (what _dequant decodes with)
    rng = np.random.default_rng(8 + bm)
    for K in (256, 768):
        for N in (256, 512):
            for M in (bm, bm + 8):
                A = (rng.standard_normal((M, K)) * np.exp(rng.standard_normal((M, 1)))).astype(np.float32)
                Wt = (rng.standard_normal((N, K)) * 0.05).astype(np.float32)
                out, A8, Asc, W8, Wsc = _gemm_f8(A, Wt, PP_TILE[bm])
                ref = _dequant(A8, Asc, M) @ _dequant(W8, Wsc, N).T
                err = np.abs(out - ref).max() / np.abs(ref).max()
                print(f"  fp8 pp {bm} M {M} N {N} K {K}: max err / max |ref| = {err:.3g}")
                assert err < 5e-4, (bm, M, N, K, err)                      # the bound of test_gpu_fp8.py
                big = _gemm_f8(A, Wt, PP_TILE[256])[0]
                assert np.array_equal(out.view(np.uint32), big.view(np.uint32)), (bm, M, N, K)


@pytest.mark.parametrize("bm", [128, 160])
def test_split_form_of_the_small_tiles(bm):
    """Precision 4 sends M <= 256 to its skinny kernel, so the smallest launches of the ping-pong form are two tiles
    + 8 rows (a third tile of clamped rows) and three whole tiles.  K = 64 is the form's two K-tiles (32 k-values each)."""
    rng = np.random.default_rng(4 + bm)
    for K in (64, 128, 768):
        for N in (256, 512):
            for M in (2 * bm + 8, 3 * bm):
                d = make_gemm(rng, R.EPI_RESID, M, N, K)
                label = f"split pp {bm} M {M} N {N} K {K}"
                out = check_gemm(4, R.EPI_RESID, d, label, tile=bm, a_scale=2.0, w_scale=4.0)[1]
                assert np.array_equal(out.view(np.uint8), run_bytes(4, R.EPI_RESID, d, -1, a_scale=2.0, w_scale=4.0, out_scale=4.0)), label
