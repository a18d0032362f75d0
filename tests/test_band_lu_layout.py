"""The band-storage LU's layout (gls_band_lu_layout): block width, block count and element count, host only."""
import pytest

from softx_2020_200_amd.native import GLSError, band_lu_layout

# (n, bl, bu, block) -> (nb, n_blocks, n_floats = 3 n nb)
CASES = [
    ((1000, 100, 100, 128), (128, 8, 3 * 1000 * 128)),
    ((777, 37, 200, 256), (256, 4, 3 * 777 * 256)),
    ((515, 0, 60, 128), (128, 5, 3 * 515 * 128)),
    ((515, 60, 0, 128), (128, 5, 3 * 515 * 128)),
    ((300, 250, 250, 256), (256, 2, 3 * 300 * 256)),
    ((100, 20, 20, 128), (128, 1, 3 * 100 * 128)),
    ((256, 30, 30, 128), (128, 2, 3 * 256 * 128)),
    # automatic: the band rounded up to a multiple of 256, at least 512
    ((1000, 100, 100, 0), (512, 2, 3 * 1000 * 512)),
    ((25000, 1900, 1850, 0), (2048, 13, 3 * 25000 * 2048)),
    ((85000, 6600, 6500, 0), (6656, 13, 3 * 85000 * 6656)),
    ((5000, 512, 513, 0), (768, 7, 3 * 5000 * 768)),
    ((1, 0, 0, 0), (512, 1, 3 * 512)),
    # past 2^31 elements: exact in 64 bits
    ((400000, 8000, 8000, 0), (8192, 49, 9830400000)),
]


@pytest.mark.parametrize("args,want", CASES)
def test_layout(args, want):
    assert band_lu_layout(*args) == want
    assert want[2] == 3 * args[0] * want[0]
    assert want[0] >= max(args[1], args[2], 1) and want[0] % 128 == 0


def test_layout_past_int32():
    nb, nblk, nfl = band_lu_layout(400000, 8000, 8000)
    assert nfl > 2**31 and nfl == 3 * 400000 * nb and nblk == -(-400000 // nb)


@pytest.mark.parametrize("args", [
    (0, 0, 0, 0), (-5, 1, 1, 0),            # n <= 0
    (100, -1, 3, 0), (100, 3, -1, 0),       # negative bandwidths
    (100, 3, 3, 64), (100, 3, 3, 127),      # block < 128
    (100, 3, 3, 192), (1000, 3, 3, 300),    # not a multiple of 128
    (1000, 200, 3, 128), (1000, 3, 200, 128),  # narrower than the band
    (100, 100, 3, 0),                       # a bandwidth outside the matrix
])
def test_layout_refusals(args):
    with pytest.raises(GLSError, match="gls_band_lu_layout"):
        band_lu_layout(*args)
