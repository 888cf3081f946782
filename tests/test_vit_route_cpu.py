"""The GEMM dispatch of the ViT block (vit_gemm.hip route_vit_gemm, reached host-only through pio_test_gemm_route), pinned to the table
the thresholds in vit_gemm.hip state for ViT-B at 224^2 (Tp = 264).  The float64 tests of tests/test_gpu_vit_kernels.py hold each path on
its own; this table says which of them a forward actually runs, and changes only on purpose when a threshold changes.

    images   qkv     fc1       proj / fc2
    16       K256    K256      NARROW          (51 tiles of 256 x 256: below the 144 the 256-wide kernels need)
    48       K256    WIDE128   ROLL            (fc1: 600 tiles = 2.34 rounds of 256 CUs, the 256 kernel's near-empty last round)
    64       K256    ROLL      ROLL            (fc1: 792 tiles >= the rolling kernel's 704 comes before the 256 kernel's 3.09-round
                                                exception, which therefore serves 48 images rather than 64)
    80, 160  ROLL    ROLL      ROLL
"""
import pytest

from patchioner_amd import _lib

PE, QKV, RES, GELU = 0, 1, 2, 3
NARROW, RES128, WIDE128, K256, ROLL = 1, 2, 3, 4, 5
D, TP = 768, 264


@pytest.fixture(scope="module")
def lib():
    from patchioner_amd import build
    build.build()
    return _lib.load()


def _route(lib, epi, imgs, N, K, D=D, Tp=TP, capture=False):
    return lib.pio_test_gemm_route(epi, imgs * Tp, N, K, K, D, Tp, int(capture))


@pytest.mark.parametrize("imgs,qkv,fc1,proj,fc2", [
    (16, K256, K256, NARROW, NARROW),
    (48, K256, WIDE128, ROLL, ROLL),
    (64, K256, ROLL, ROLL, ROLL),
    (80, ROLL, ROLL, ROLL, ROLL),
    (160, ROLL, ROLL, ROLL, ROLL),
])
def test_vit_b_224_dispatch_table(lib, imgs, qkv, fc1, proj, fc2):
    assert _route(lib, QKV, imgs, 3 * D, D) == qkv
    assert _route(lib, GELU, imgs, 4 * D, D) == fc1
    assert _route(lib, RES, imgs, D, D) == proj
    assert _route(lib, RES, imgs, D, 4 * D) == fc2


@pytest.mark.parametrize("imgs", [1, 16, 64, 80, 160, 320])
def test_last_block_qkv_with_capture_never_rolls(lib, imgs):
    p = _route(lib, QKV, imgs, 3 * D, D, capture=True)
    assert p in (WIDE128, K256)


@pytest.mark.parametrize("imgs", [1, 16, 32, 64, 80, 160, 320])
@pytest.mark.parametrize("Tp", [264, 1376])
def test_vit_s_proj_never_takes_a_lazy_join(lib, imgs, Tp):
    """ViT-S proj: K = 384, six K-tiles, fewer than the lazy x join's ten: always the eager narrow form."""
    assert _route(lib, RES, imgs, 384, 384, D=384, Tp=Tp) == NARROW


def test_residual_lazy_form_only_from_ten_k_tiles(lib):
    for K, want in ((512, NARROW), (640, RES128)):     # 128 images x 264 rows of N = 768: 396 tiles of 128 x 128 (>= 384)
        assert lib.pio_test_gemm_route(RES, 128 * TP, 768, K, K, 768, TP, 0) == want


def test_sizes_no_kernel_takes_are_refused(lib):
    assert lib.pio_test_gemm_route(RES, 264, 768, 100, 100, 768, TP, 0) == -1     # K % 128 != 0
    assert lib.pio_last_error()
    assert lib.pio_test_gemm_route(QKV, 264, 2300, 768, 768, 768, TP, 0) == -1    # N != 3 D
    assert lib.pio_test_gemm_route(7, 264, 768, 768, 768, 768, TP, 0) == -1
