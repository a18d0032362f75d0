"""Boundary face list of an FE space (gls_fe_space_boundary_faces through FESpaceHandle.boundary_faces):
the faces, normals, JxW and mapped points the force / torque integrals of the reference run over
(postprocessing_force.cc, postprocessing_torque.cc: every at_boundary() face of the active cells,
QGauss<dim-1>(k + 1), MappingQ(k)). Host-only (CPU) tests:
  * unit square / cube: face counts, unit areas per id, normals +-e_d, points on the right plane;
  * closed surface: sum over all boundary faces of n JxW = 0 on conforming curved meshes (exact: the
    integrand dx/du x dx/dv of a Q2 face has degree 3 per variable and Gauss(3) integrates it exactly);
  * the perimeters of the hyper_shell converge to 2 pi r at the rate of the Q2 mapping;
  * adapted meshes: the list equals the walk over the space's cells, every active boundary face once."""
import os

import numpy as np
import pytest

from softx_2020_200_amd.native import UMesh
from tests.test_uforest import CASES

HERE = os.path.dirname(os.path.abspath(__file__))
MESHES = os.path.join(HERE, "golden", "meshes")


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("k,kp", [(1, 1), (2, 1)])
def test_unit_cube_faces(dim, k, kp):
    m = UMesh(dim, "hyper_cube", "0 : 1 : true")
    m.refine_global(1)
    f = m.fe_space_handle(k, kp).boundary_faces(k + 1)
    assert len(f["cell"]) == 2 * dim * 2 ** (dim - 1)
    assert f["nqf"] == (k + 1) ** (dim - 1)
    assert sorted(set(f["id"])) == list(range(2 * dim))
    for bid in range(2 * dim):  # colorize: id = 2 d + side
        d, s = bid // 2, bid % 2
        on = f["id"] == bid
        assert np.array_equal(f["face"][on], np.full(on.sum(), bid))
        assert abs(f["jxw"][on].sum() - 1.0) <= 1e-14
        n = np.zeros(dim)
        n[d] = 1.0 if s else -1.0
        assert np.abs(f["normal"][on] - n).max() <= 1e-14
        assert np.abs(f["xq"][on][..., d] - s).max() <= 1e-14
        assert np.abs(f["xi"][on][..., d] - s).max() == 0.0
    # jinv of a box cell: diag(1 / h), h = 1/2
    assert np.abs(f["jinv"] - 2.0 * np.eye(dim)).max() <= 1e-13


def closed_meshes():
    def shell(r):
        m = UMesh(2, "hyper_shell", "0, 0 : 0.25 : 1 : 4 : true")
        m.refine_global(r)
        return m
    return [("shell4", lambda: shell(0)), ("shell4_refined", lambda: shell(1)),
            ("cylinder_shell", lambda: UMesh(3, "cylinder_shell", "0.5 : 0.25 : 1 : 8 : 2")),
            ("cylinder3d_1layer", lambda: UMesh(3, gmsh=os.path.join(MESHES, "cylinder3d_1layer.msh")))]


@pytest.mark.parametrize("name,make", closed_meshes(), ids=[c[0] for c in closed_meshes()])
def test_closed_surface(name, make):
    m = make()
    f = m.fe_space_handle(2, 1).boundary_faces(3)
    assert len(f["cell"]) > 0
    area = f["jxw"].sum()
    s = (f["normal"] * f["jxw"][..., None]).sum(axis=(0, 1))
    print(name, "faces", len(f["cell"]), "area", area, "sum n JxW", s)
    assert np.abs(s).max() <= 1e-13 * area
    assert np.abs(np.linalg.norm(f["normal"], axis=-1) - 1.0).max() <= 1e-14


def test_shell_perimeters_converge():
    err = []
    for r in range(3):
        m = UMesh(2, "hyper_shell", "0, 0 : 0.25 : 1 : 4 : true")
        m.refine_global(r)
        f = m.fe_space_handle(2, 1).boundary_faces(3)
        err.append([abs(f["jxw"][f["id"] == 0].sum() - 2 * np.pi * 0.25), abs(f["jxw"][f["id"] == 1].sum() - 2 * np.pi)])
        # the points lie near the circles and the normals are radial (outward of the domain)
        for bid, rad, sign in ((0, 0.25, -1.0), (1, 1.0, 1.0)):
            on = f["id"] == bid
            x, n = f["xq"][on].reshape(-1, 2), f["normal"][on].reshape(-1, 2)
            assert np.abs(np.linalg.norm(x, axis=1) - rad).max() < 2e-2 * rad
            assert ((x * n).sum(axis=1) * sign > 0.9 * rad).all()
    print("perimeter errors (id 0, id 1) per refinement:", err)
    for a, b in zip(err[:-1], err[1:]):  # nominal 16x for the Q2 arc
        assert b[0] <= a[0] / 8 and b[1] <= a[1] / 8, err


def walk_boundary_faces(sp):
    """(cell, face, id) of the faces whose Q2 face nodes all carry one boundary id bit (the face's middle
    node lies on the boundary only when the face does)"""
    dim, k = sp["dim"], sp["k"]
    assert k == 2
    k1 = k + 1
    out = []
    for c in range(sp["n_cells"]):
        for fc in range(2 * dim):
            d, s = fc // 2, fc % 2
            bits = 0xFFFFFFFF
            for a in range(k1 ** dim):
                if (a // k1 ** d) % k1 == s * k:
                    bits &= int(sp["vnode_bid"][sp["cell_vnodes"][c, a]])
            if bits:
                assert bits & (bits - 1) == 0, (c, fc, bits)
                out.append((c, fc, bits.bit_length() - 1))
    return out


@pytest.mark.parametrize("name,dim,spec,flat", [CASES[1], CASES[3]], ids=[CASES[1][0], CASES[3][0]])
def test_adapted_mesh_faces(name, dim, spec, flat):
    from tests.test_gpu_uforest import adapted_space  # host-only helper (no device call)
    m, h = adapted_space(name, dim, spec, 2, 1)
    sp = h.data
    assert sp["vhang"], "no hanging nodes"
    f = h.boundary_faces(3)
    listed = list(zip(f["cell"].tolist(), f["face"].tolist(), f["id"].tolist()))
    assert min(f["cell"]) >= 0 and max(f["cell"]) < sp["n_cells"]
    assert len(set((c, fc) for c, fc, _ in listed)) == len(listed)  # each face once
    assert sorted(listed) == sorted(walk_boundary_faces(sp))
    # the boundary is covered once: the areas per id equal those of the unadapted (refined once) mesh
    from tests.test_uforest import make_mesh
    m0 = make_mesh(dim, spec)
    m0.refine_global(1)
    f0 = m0.fe_space_handle(2, 1, qmapping_all=True).boundary_faces(3)
    for bid in sorted(set(f0["id"])):
        a, a0 = f["jxw"][f["id"] == bid].sum(), f0["jxw"][f0["id"] == bid].sum()
        assert abs(a - a0) < 2e-2 * a0, (bid, a, a0)  # finer faces follow the curved boundary more closely
