"""Pointwise limb GEMMs for channel widths in steps of 32 - what can be checked without a GPU: the new predicates of the C
ABI beside the unchanged old ones, the byte count of the padded fragment sets, the work items of the batched packer, and
the route functions (score_routes.pointwise_route / pointwise_wgrad_route) on the shapes of the nf = 160 AFHQv2-128
inpainting network and of the C10 network."""
import pytest

from psld_amd import _lib
from psld_amd import score_routes as R

TAIL_KN = [(160, 160), (320, 480), (480, 1440), (960, 480), (2880, 320)]


def test_tail_predicates():
    lib = _lib.load()
    assert lib.psld_version() == _lib.ABI_VERSION == 14
    for k, n in TAIL_KN:
        for m in (1, 130, 4 * 16 * 16, 16 * 128 * 128):
            assert lib.psld_gemm_tail_supported(k, m, n) == 1, (k, m, n)
            assert lib.psld_gemm_split_supported(k, 0, m, n) == 0, (k, m, n)
    m = 4096
    for k, n in ((160, 96), (160, 144), (176, 160), (96, 160), (160, 0), (0, 160)):
        assert lib.psld_gemm_tail_supported(k, m, n) == 0, (k, n)
    assert lib.psld_gemm_tail_supported(160, 0, 160) == 0
    # every shape the old predicate takes stays the old kernels'
    for k, n in ((256, 256), (512, 256), (128, 128), (64, 128), (1152, 384), (320, 256)):
        assert lib.psld_gemm_split_supported(k, 0, m, n) == 1 and lib.psld_gemm_tail_supported(k, m, n) == 0, (k, n)
    # K in steps of 32 under a full-tile N, and the reverse
    assert lib.psld_gemm_tail_supported(160, m, 256) == 1 and lib.psld_gemm_tail_supported(256, m, 160) == 1

    for mm, nn in ((160, 160), (320, 480), (480, 160), (480, 1440), (128, 160), (160, 128)):
        for kk in (128, 2048, 32):
            assert lib.psld_gemm_tn_split_tail_supported(mm, nn, kk) == 1, (mm, nn, kk)
            assert lib.psld_gemm_tn_split_supported(mm, nn, kk) == 0
    for mm, nn, kk in ((96, 160, 128), (160, 96, 128), (144, 160, 128), (160, 160, 48), (160, 160, 0), (128, 128, 64), (256, 384, 64)):
        assert lib.psld_gemm_tn_split_tail_supported(mm, nn, kk) == 0, (mm, nn, kk)


def test_old_predicates_unchanged():
    """The values the existing tests pin."""
    lib = _lib.load()
    for m in (130, 1000, 64 * 32 * 32):
        assert lib.psld_gemm_split_supported(160, 0, m, 160) == 0
    assert lib.psld_gemm_split_x3_supported(160, 0, 64 * 32 * 32, 256) == 0
    assert lib.psld_gemm_tn_split_supported(64, 128, 64) == 0 and lib.psld_gemm_tn_split_supported(128, 128, 48) == 0
    assert lib.psld_gemm_tn_split_supported(128, 128, 64) == 1 and lib.psld_gemm_split_supported(256, 256, 100, 256) == 1
    assert lib.psld_gemm_frag_bytes(256, 512) == 256 * 512 * 6


def test_tail_fragment_bytes_and_items():
    lib = _lib.load()

    def up(v, g):
        return -(-v // g) * g
    for k, n in TAIL_KN + [(160, 256), (256, 160), (4320, 480)]:
        assert lib.psld_gemm_frag_bytes_tail(n, k) == up(n, 128) * up(k, 64) * 6, (n, k)
    assert lib.psld_gemm_frag_bytes_tail(256, 512) == lib.psld_gemm_frag_bytes(256, 512)
    # work items of the batched packer: one per lane slot (a row's 8 consecutive k) of the region a tensor writes; the tensor
    # that ends a dimension of the set also writes that dimension's zero padding
    assert lib.psld_pack_frag_tail_items(160, 0, 0, 160, 0, 0) == 256 * 6 * 4
    c = 160
    rows = [lib.psld_pack_frag_tail_items(c, i * c, 3 * c, c, 0, 0) for i in range(3)]         # q | k | v along N
    assert rows == [c * 6 * 4, c * 6 * 4, (512 - 2 * c) * 6 * 4]
    assert sum(rows) * 48 == lib.psld_gemm_frag_bytes_tail(3 * c, c)                         # 3 limbs x 16 bytes per item
    ks = [lib.psld_pack_frag_tail_items(c, 0, 0, c, i * 5, 15) for i in range(3)]              # ... and along K
    assert ks == [256 * 5 * 4, 256 * 5 * 4, 256 * 6 * 4]
    assert sum(ks) * 48 == lib.psld_gemm_frag_bytes_tail(c, 3 * c)


# pointwise contractions of afhqv2_128_inpaint (nf 160; widths 160 / 320 / 480 at 128 / 64, 32 / 16, 8; concatenations
# materialised): (k, n, map side) of the 1x1 shortcuts, the attention projections and the stride-2 pyramid GEMMs
AFHQ160_FWD = [
    (160, 320, 64), (320, 480, 16),                                                  # down path shortcuts
    (960, 480, 8), (960, 480, 16), (800, 480, 16), (800, 320, 32), (640, 320, 32), (640, 320, 64), (480, 320, 64),
    (480, 160, 128), (320, 160, 128),                                                # up path shortcuts
    (480, 1440, 16), (480, 480, 16), (1440, 480, 16), (480, 1440, 8), (480, 480, 8), (1440, 480, 8),   # attention
    (1440, 320, 64), (2880, 320, 32), (2880, 480, 16), (4320, 480, 8),               # pyramid, forward ...
    (320, 1440, 64), (320, 2880, 32), (480, 2880, 16), (480, 4320, 8),               # ... and data gradient
]
C10_FWD = [(128, 256, 16), (256, 256, 16), (256, 768, 16), (768, 256, 16), (512, 256, 8), (384, 128, 32), (1152, 256, 16),
           (256, 1152, 16)]


@pytest.mark.parametrize("b", [4, 16])
def test_route_table(b):
    _lib.load()
    for k, n, s in AFHQ160_FWD:
        m = b * s * s
        assert R.pointwise_route(True, k, 0, m, n) == R.LIMB_TAIL, (k, n, s)
        # its data gradient (320 -> 640 is a full-tile shape: the old kernel's, as on the parent)
        assert R.pointwise_route(True, n, 0, m, k) == (R.LIMB if (k, n) == (640, 320) else R.LIMB_TAIL), (k, n, s)
        assert R.pointwise_route(False, k, 0, m, n) == R.TILE
        # weight gradient dW[n][k] (a 1x1 convolution's) and dW[k][n] (NIN's [in][out])
        assert R.pointwise_wgrad_route(True, n, k, 0, m) == R.LIMB_TAIL and R.pointwise_wgrad_route(True, k, n, 0, m) == R.LIMB_TAIL
        assert R.pointwise_wgrad_route(False, n, k, 0, m) == R.TILE
    for k, n, s in C10_FWD:                                                               # as today
        m = b * 8 * s * s
        assert R.pointwise_route(True, k, 0, m, n) == R.LIMB, (k, n, s)
        assert R.pointwise_wgrad_route(True, n, k, 0, m) == R.LIMB, (k, n, s)
    # two sources: the old kernels or the tile engine, never the one-source tail launch
    assert R.pointwise_route(True, 256, 128, 1024, 256) == R.LIMB
    assert R.pointwise_route(True, 160, 160, 1024, 160) == R.TILE
    assert R.pointwise_wgrad_route(True, 256, 256, 128, 1024) == R.LIMB
    assert R.pointwise_wgrad_route(True, 160, 160, 160, 1024) == R.TILE
    # widths no limb kernel takes
    for k, n in ((96, 160), (160, 96), (160, 144), (176, 160), (54, 160)):
        assert R.pointwise_route(True, k, 0, 1024, n) == R.TILE, (k, n)
    assert R.pointwise_wgrad_route(True, 160, 96, 0, 1024) == R.TILE
    # K ranges of the weight gradient count cut tiles as tiles
    assert R._tn_split(256, 256, 4096) == R._tn_split(160, 160, 4096)
