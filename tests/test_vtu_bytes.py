"""write_vtu pinned byte for byte: the files under tests/golden/vtu/ were written by the library before the
base64 encoder wrote straight into one preallocated buffer and before gls_vtu_write shared its file writer
with gls_vtu_write_device. Binary and ASCII, a 2x1-cell 2D Q2-Q1 mesh (Lagrange cells, subdivision 2, SRF:
every array the writer knows) and a 2-cell 3D Q1-Q1 mesh (linear cells, subdivision 1). The array lengths
leave 0, 1 and 2 bytes over after the last full base64 triple, so every padding branch is in the files."""
import os

import numpy as np
import pytest

from softx_2020_200_amd.io import write_vtu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vtu")


def row_mesh(dim, n_x, k, kp, x0, h):
    """n_x cells in a row along x (one cell thick in the other directions): the hyper_cube dict layout, the
    nodes of each space numbered lexicographically on the row's lattice"""
    def space(m):
        n1 = [m * n_x + 1] + [m + 1] * (dim - 1)
        cells = np.zeros((n_x, (m + 1) ** dim), dtype=np.int32)
        for c in range(n_x):
            for a in range((m + 1) ** dim):
                ia = [(a // (m + 1) ** d) % (m + 1) for d in range(dim)]
                ia[0] += m * c
                cells[c, a] = ia[0] + n1[0] * (ia[1] + n1[1] * (ia[2] if dim == 3 else 0))
        return cells, int(np.prod(n1))
    cv, nv = space(k)
    cp, npn = space(kp)
    cx0 = np.array([[x0[0] + c * h[0]] + list(x0[1:dim]) for c in range(n_x)])
    return dict(dim=dim, k=k, kp=kp, n_cells=n_x, n_vnodes=nv, n_pnodes=npn, cell_vnodes=cv, cell_pnodes=cp,
                cell_x0=cx0, cell_h=np.tile(np.asarray(h[:dim], dtype=np.float64), (n_x, 1)))


def field(n):
    """a fixed vector with no short binary expansion, independent of any random generator"""
    i = np.arange(n, dtype=np.float64)
    return ((i * 0.6180339887498949 + 0.1234567) % 1.0) * 2.0 - 1.0


CASES = {
    "q2q1_2d_2x1": dict(mesh=row_mesh(2, 2, 2, 1, (0.25, -0.5), (0.375, 0.7)), subdivision=2, subdomain=3, srf=True,
                        omega=(0.0, 0.0, 0.5)),
    "q1q1_3d_2": dict(mesh=row_mesh(3, 2, 1, 1, (-1.0, 0.1, 0.3), (0.3, 0.45, 1.1)), subdivision=1, subdomain=0, srf=False,
                      omega=(0.0, 0.0, 0.0)),
}


def write_case(name, binary, path):
    c = CASES[name]
    m = c["mesh"]
    sol = field(m["dim"] * m["n_vnodes"] + m["n_pnodes"])
    write_vtu(path, m, sol, subdivision=c["subdivision"], subdomain=c["subdomain"], binary=binary, srf=c["srf"],
              omega=c["omega"])


@pytest.mark.parametrize("binary", [True, False], ids=["binary", "ascii"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_write_vtu_bytes(tmp_path, name, binary):
    f = str(tmp_path / "out.vtu")
    write_case(name, binary, f)
    with open(f, "rb") as a, open(os.path.join(GOLDEN, "%s_%s.vtu" % (name, "binary" if binary else "ascii")), "rb") as b:
        got, want = a.read(), b.read()
    assert len(want) < 64 * 1024
    assert got == want
