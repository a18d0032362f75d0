"""GPU: the band-storage FP32 LU on its own (gls_band_lu_*) against numpy.

Matrices: rows U(-1, 1) inside the band (seeded), the diagonal the row's absolute sum plus 1, handed over as an FP64 CSR
WITHOUT the pin; the library replaces row and column `pin` by identity, the reference does the same in numpy. An FP32
unpivoted LU of these is benign (in numpy: relative errors against the FP64 solve 3e-8 .. 9e-7, check values
5e-8 .. 4e-7, condition numbers 3e1 .. 2e2).

Bounds: the device solve against numpy.linalg.solve in FP64 may be off by 4 x the error of a numpy float32 unpivoted LU
of the same matrix (lu32 / lu32_solve below: the same arithmetic in another summation order), the project's 4 x
convention; with refine=1 by 4 x the error of the numpy restatement of one refinement step, and by less than the
unrefined solve."""
import functools

import numpy as np
import pytest

from gpu_util import cuda

# (n, bl, bu, block)
SHAPES = [
    (1000, 100, 100, 128),  # partial last block, 8 blocks
    (777, 37, 200, 256),    # bl != bu, odd n: the scalar loads
    (515, 0, 60, 128),      # upper triangular band
    (515, 60, 0, 128),      # lower triangular band
    (300, 250, 250, 256),   # the band covers most of the matrix
    (100, 20, 20, 128),     # one block
    (256, 30, 30, 128),     # n = 2 nb exactly
]
PINS = ["first", "last", "boundary", "none"]
SEED = 20200200


def pin_of(shape, where):
    n, _, _, block = shape
    return {"first": 0, "last": n - 1, "boundary": block if block < n else n // 2, "none": -1}[where]


@functools.lru_cache(maxsize=None)
def dense(shape):
    n, bl, bu, _ = shape
    rng = np.random.default_rng(SEED + n + 7 * bl + 13 * bu)
    i, j = np.indices((n, n))
    band = (i - j <= bl) & (j - i <= bu)
    A = np.where(band, rng.uniform(-1, 1, (n, n)), 0.0)
    A[i == j] = 0.0
    A[i == j] = np.abs(A).sum(axis=1) + 1.0
    b = rng.uniform(-1, 1, n)
    A.setflags(write=False), b.setflags(write=False), band.setflags(write=False)
    return A, b, band


def csr_of(A, band):
    """every position of the band is an entry (zeros included would change nothing: the values are nonzero a.s.)"""
    n = A.shape[0]
    rowp = np.concatenate([[0], np.cumsum(band.sum(axis=1))]).astype(np.int64)
    r, c = np.nonzero(band)  # row-major: rows ascending, columns ascending inside a row
    return rowp, c.astype(np.int32), A[r, c].copy()


def pinned(A, pin):
    Ap = A.copy()
    if pin >= 0:
        Ap[pin, :] = 0.0
        Ap[:, pin] = 0.0
        Ap[pin, pin] = 1.0
    return Ap


def lu32(Ap, bl, bu):
    """numpy float32 unpivoted LU (in place, unit L below the diagonal), inside the band"""
    n = Ap.shape[0]
    M = Ap.astype(np.float32)
    for k in range(n - 1):
        r1, c1 = min(n, k + bl + 1), min(n, k + bu + 1)
        M[k + 1:r1, k] = M[k + 1:r1, k] / M[k, k]
        M[k + 1:r1, k + 1:c1] -= np.outer(M[k + 1:r1, k], M[k, k + 1:c1])
    return M


def lu32_solve(M, b):
    n = M.shape[0]
    x = b.astype(np.float32)
    for k in range(n):  # column-oriented forward, then backward substitution in float32
        x[k + 1:] -= M[k + 1:, k] * x[k]
    for k in range(n - 1, -1, -1):
        x[k] = x[k] / M[k, k]
        x[:k] -= M[:k, k] * x[k]
    return x


@functools.lru_cache(maxsize=None)
def reference(shape, where):
    """the FP64 solution with x[pin] = 0, and the numpy float32 restatement's errors (plain / one refinement step)"""
    n, bl, bu, _ = shape
    A, b, _ = dense(shape)
    pin = pin_of(shape, where)
    Ap = pinned(A, pin)
    x = np.linalg.solve(Ap, b)
    M = lu32(Ap, bl, bu)
    x0 = lu32_solve(M, b).astype(np.float64)
    x1 = x0 + lu32_solve(M, b - Ap @ x0).astype(np.float64)
    if pin >= 0:
        x[pin] = x0[pin] = x1[pin] = 0.0
    scale = np.abs(x).max()
    chk = np.linalg.norm(Ap @ lu32_solve(M, np.where(np.arange(n) == pin, 0.0, 1.0)).astype(np.float64) -
                         np.where(np.arange(n) == pin, 0.0, 1.0)) / np.sqrt(n)
    x.setflags(write=False)
    return x, np.abs(x0 - x).max() / scale, np.abs(x1 - x).max() / scale, chk


@pytest.mark.gpu
@pytest.mark.parametrize("where", PINS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d-bl%d-bu%d-b%d" % s)
def test_band_lu_solve(shape, where):
    import torch
    from softx_2020_200_amd.native import BandLU, band_lu_layout
    n, bl, bu, block = shape
    A, b, band = dense(shape)
    pin = pin_of(shape, where)
    x_ref, e_np, e_np_ref, chk_np = reference(shape, where)
    lu = BandLU(*csr_of(A, band), pin=pin, block=block)
    info = lu.info()
    nb, nblk, nfl = band_lu_layout(n, bl, bu, block)
    assert (info["bl"], info["bu"], info["nb"], info["bytes"]) == (bl, bu, nb, 4 * nfl), info
    B = cuda(b)
    x = lu.solve(B)
    again = lu.solve(B)
    xr = lu.solve(B, refine=True)
    xr_again = lu.solve(B, refine=True)
    torch.cuda.synchronize()
    scale = np.abs(x_ref).max()
    e = np.abs(x.cpu().numpy() - x_ref).max() / scale
    er = np.abs(xr.cpu().numpy() - x_ref).max() / scale
    print("band LU n=%d bl=%d bu=%d nb=%d (%d blocks) pin=%d: rel err %.3e (numpy f32 LU %.3e), refined %.3e (numpy %.3e), "
          "check %.3e (numpy %.3e)" % (n, bl, bu, nb, nblk, pin, e, e_np, er, e_np_ref, info["check"], chk_np))
    assert np.isfinite(x.cpu().numpy()).all() and np.isfinite(xr.cpu().numpy()).all()
    assert torch.equal(x, again) and torch.equal(xr, xr_again)  # fixed summation order
    if pin >= 0:
        assert float(x[pin]) == 0.0 and float(xr[pin]) == 0.0
    assert e <= 4 * e_np, (e, e_np)
    assert er <= 4 * e_np_ref, (er, e_np_ref)
    assert er < e, (er, e)
    assert info["check"] < 1e-2, info["check"]  # (benign matrices: the factor is used without refinement)
    lu.close()


@pytest.mark.gpu
def test_in_place_solve_and_input_untouched():
    """b == x is allowed (the coarse solve works in place); a separate b is not written"""
    import ctypes as C
    import torch
    from softx_2020_200_amd.native import BandLU, check
    shape = (256, 30, 30, 128)
    A, b, band = dense(shape)
    lu = BandLU(*csr_of(A, band), pin=5, block=128)
    B = cuda(b)
    keep = B.clone()
    x = lu.solve(B, refine=True)
    assert torch.equal(B, keep)
    check(lu.L.gls_band_lu_solve(lu.h, C.c_void_p(B.data_ptr()), C.c_void_p(B.data_ptr()), 1), "gls_band_lu_solve")
    assert torch.equal(B, x)


@pytest.mark.gpu
def test_singular_second_block_is_refused_at_create():
    """a zero row inside the second 128-block: the unpivoted factor breaks there, the check is not finite (or O(1)),
    and create refuses with GLS_EINVAL naming it -- there is no pivoted route in band storage"""
    from softx_2020_200_amd.native import BandLU, GLSError
    shape = (300, 20, 20, 128)
    A, _, band = dense(shape)
    A = A.copy()
    A[130, :] = 0.0
    with pytest.raises(GLSError) as ei:
        BandLU(*csr_of(A, band), pin=0, block=128)
    msg = str(ei.value)
    print(msg)
    assert "(-1)" in msg and "failed its check" in msg, msg
    val = float(msg.split("|A x - 1| / |1| =")[1].split()[0])
    assert not np.isfinite(val) or val >= 0.5, val


@pytest.mark.gpu
def test_create_refusals():
    from softx_2020_200_amd.native import BandLU, GLSError
    A, _, band = dense((100, 20, 20, 128))
    rowp, col, val = csr_of(A, band)
    with pytest.raises(GLSError, match="narrower than the band"):
        BandLU(*csr_of(*dense((300, 250, 250, 256))[::2]), block=128)
    with pytest.raises(GLSError, match="multiple of 128"):
        BandLU(rowp, col, val, block=100)
    bad = col.copy()
    bad[3] = 100
    with pytest.raises(GLSError, match="column out of range"):
        BandLU(rowp, bad, val)
    with pytest.raises(GLSError, match="pin"):
        BandLU(rowp, col, val, pin=100)
