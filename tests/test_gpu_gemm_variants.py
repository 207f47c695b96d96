"""Every fp16 GEMM tile variant computes bit-identical results (same MFMAs in the same k order): the
ping-pong kernel's tile heights, its planner (uniform / tail-balanced grids) and the 16-wave kernels against
the 128x128 baseline, on shapes with ragged M, the minimum K (two K-tiles), long K and many column tiles."""
import ctypes as C

import pytest

from cbas_amd import _lib

pytestmark = pytest.mark.gpu

SHAPES = [(300, 256, 128), (1000, 512, 256), (257, 256, 4096), (5000, 1024, 1024), (12864, 768, 768), (6432, 3072, 768),
          (12864, 2304, 768), (32928, 1024, 1024), (1, 256, 768), (64, 768, 3072), (37, 3072, 768)]
TILES = [4, 7, 13, 14, 15, 16, 17]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_tile_variants_are_bit_identical(shape):
    lib = _lib.load()
    fn = lib.cbas_debug_gemm_bench
    m, n, k = shape

    def run(tile):
        ms, cs = C.c_float(), C.c_ulonglong()
        _lib.check(fn(m, n, k, tile, 1, C.byref(ms), C.byref(cs)), f"gemm tile {tile}")
        return cs.value

    ref = run(1)
    assert ref != 0
    for t in TILES + ([8, 9] if m <= 64 else []):            # 64x128 and the skinny ring kernel for the CLS-row GEMMs
        assert run(t) == ref, (shape, t)


@pytest.mark.parametrize("epi", ["resid", "qkv"])
@pytest.mark.parametrize("shape", [(1000, 768, 256), (12865, 768, 768), (300, 2304, 768)], ids=lambda s: "x".join(map(str, s)))
def test_tile_variants_are_bit_identical_on_residual_and_qkv_epilogues(epi, shape):
    """The same through cbas_debug_gemm_run with non-zero bias, lambda, residual x and real RoPE tables (the bench above
    only runs the GELU epilogue on a zero bias): every tile form's bytes equal the 128x128 kernel's."""
    import numpy as np
    from oracle import kernel_ref as R
    from test_gpu_kernel_reference import gemm_run, make_gemm, out_buffer

    m, n, k = shape
    e = R.EPI_RESID if epi == "resid" else R.EPI_QKV
    d = make_gemm(np.random.default_rng(m + n), e, m, n, k, frames_P=(14, 14))

    def run(tile, rope_lds=0):
        return gemm_run(0, e, d["A"], d["W"], d["bias"], M=m, out=out_buffer(0, e, d), tile=tile, lam=d.get("lam"),
                        cos=d.get("cos"), sin=d.get("sin"), D=d.get("D", 0), T=d.get("T", 0), n_prefix=d.get("n_prefix", 0),
                        P=d.get("P", 0), nh=d.get("nh", 0), nw=d.get("nw", 0), rope_lds=rope_lds)

    ref = run(1)
    for t in TILES:
        for lds in ((0, 1) if e == R.EPI_QKV and t >= 13 else (0,)):
            assert np.array_equal(run(t, lds).view(np.uint8), ref.view(np.uint8)), (shape, epi, t, lds)
