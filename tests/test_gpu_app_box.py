"""GPU: apps/gls_navier_stokes --box-path brick on a subdivided_hyper_rectangle (2,1,1 subdivisions of the box
0 : (2, 1, 1), initial refinement 2: 8 x 4 x 4 cells, Q2-Q2, BDF1, two steps, the lid y = 1 moving in x and no-slip
elsewhere) against the default (general-mesh) path on the same prm; and the fallback when a condition of the box
path fails.

The tolerance of the comparison is measured, not chosen: d0 is the difference that the two solvers of the default
path (--precond ilu and --precond jacobi) show on this very case, per quantity (the printed kinetic energy and
enstrophy, the final velocity DoFs, the final pressure DoFs with their mean taken out: the enclosed box fixes the
pressure up to a constant), the DoFs of the two numberings matched by support point; the box path may differ from the
default path by 4 d0."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(ROOT, "apps", "gls_navier_stokes")
GRID = "2,1,1 : 0,0,0 : 2,1,1 : true"
CELLS, P2, K = (8, 4, 4), (2.0, 1.0, 1.0), 2

PRM = """
subsection simulation control
  set method                  = bdf1
  set time step               = 0.05
  set time end                = 0.1
  set output name             = box
  set output frequency        = 1000000
end
subsection physical properties
  set kinematic viscosity     = 0.01
end
subsection mesh
  set type                    = dealii
  set grid type               = subdivided_hyper_rectangle
  set grid arguments          = %(grid)s
  set initial refinement      = %(refinement)d
end
subsection boundary conditions
  set number = 6
  subsection bc 0
    set id = 0
    set type = noslip
  end
  subsection bc 1
    set id = 1
    set type = noslip
  end
  subsection bc 2
    set id = 2
    set type = noslip
  end
  subsection bc 3
    set id = 4
    set type = noslip
  end
  subsection bc 4
    set id = 5
    set type = noslip
  end
  subsection bc 5
    set id = 3
    set type = function
    subsection u
      set Function expression = 1
    end
    subsection v
      set Function expression = 0
    end
    subsection w
      set Function expression = 0
    end
  end
end
subsection FEM
  set velocity order          = 2
  set pressure order          = 2
end
subsection initial conditions
  set type                    = nodal
  subsection uvwp
    set Function expression   = 0; 0; 0; 0
  end
end
subsection post-processing
  set verbosity               = verbose
  set calculate kinetic energy = true
  set calculate enstrophy     = true
end
subsection non-linear solver
  set tolerance               = 1e-9
  set max iterations          = 10
  set verbosity               = quiet
end
subsection linear solver
  set method                  = gmres
  set max iters               = 1000
  set relative residual       = 1e-8
  set minimum residual        = 1e-14
  set verbosity               = quiet
end
"""


KELLY = """
subsection mesh adaptation
  set type                    = kelly
  set variable                = velocity
  set fraction refinement     = 0.1
  set fraction coarsening     = 0.0
  set frequency               = 2
end
"""


def run(tmp_path, tag, *extra, grid=GRID, refinement=2, more=""):
    d = tmp_path / tag
    d.mkdir()
    (d / "case.prm").write_text(PRM % dict(grid=grid, refinement=refinement) + more)
    (d / "dump").mkdir()
    if not os.path.exists(APP):
        pytest.fail("apps/gls_navier_stokes is not built (run __graft_entry__.build())")
    out = subprocess.run([APP, "--dim", "3", "--precision", "12", "--stats", "--dump", str(d / "dump"), *extra, "case.prm"],
                         cwd=str(d), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:] + out.stdout[-2000:]
    vals = lambda key: np.array([float(l.split(":")[1]) for l in out.stdout.splitlines() if l.startswith(key)])
    last = sorted(f for f in os.listdir(d / "dump") if f.endswith(".bin"))[-1]
    meta = dict(l.split(" ", 1) for l in open(d / "dump" / last.replace(".bin", ".meta")).read().splitlines())
    n = int(meta["n_dofs"])
    state = np.fromfile(d / "dump" / last, dtype=np.float64)[:n]
    return dict(kinetic=vals("Kinetic energy :"), enstrophy=vals("Enstrophy  :"), state=state, stderr=out.stderr,
                stdout=out.stdout, steps=int(meta["step"]))


def lattice_index(X):
    """support point -> index on the box path's lexicographic Q2 lattice (x fastest)"""
    ijk = np.rint(np.asarray(X) * (K * np.asarray(CELLS) / np.asarray(P2))).astype(np.int64)
    shape = [K * c + 1 for c in CELLS]
    assert (ijk >= 0).all() and (ijk < shape).all()
    return ijk[:, 0] + shape[0] * (ijk[:, 1] + shape[1] * ijk[:, 2])


def general_to_lattice():
    """the general path's node numbering (the library's FE space on the refined triangulation, as the application
    builds it) as lattice indices: a permutation of the box path's nodes"""
    from softx_2020_200_amd.native import UMesh
    um = UMesh(3, "subdivided_hyper_rectangle", GRID)
    um.refine_global(2)
    sp = um.fe_space(K, K)
    perm = lattice_index(sp["vnode_x"])
    assert len(np.unique(perm)) == len(perm) == int(np.prod([K * c + 1 for c in CELLS]))
    return perm


def split(state, nv, perm=None):
    """(velocity [nv, 3], mean-free pressure [nv]) in lattice order"""
    vel, p = state[:3 * nv].reshape(nv, 3), state[3 * nv:]
    if perm is not None:
        v2, p2 = np.empty_like(vel), np.empty_like(p)
        v2[perm], p2[perm] = vel, p
        vel, p = v2, p2
    return vel, p - p.mean()


def differences(a, b):
    return dict(kinetic=float(np.abs(a["kinetic"] - b["kinetic"]).max()),
                enstrophy=float(np.abs(a["enstrophy"] - b["enstrophy"]).max()),
                velocity=float(np.abs(a["vel"] - b["vel"]).max()), pressure=float(np.abs(a["p"] - b["p"]).max()))


@pytest.mark.gpu
def test_box_path_matches_the_default_path(tmp_path):
    perm = general_to_lattice()
    nv = len(perm)
    runs = {"brick": run(tmp_path, "brick", "--box-path", "brick"), "default": run(tmp_path, "default"),
            "ilu": run(tmp_path, "ilu", "--precond", "ilu"), "jacobi": run(tmp_path, "jacobi", "--precond", "jacobi")}
    for tag, r in runs.items():
        # the tables: one line per solved step (and one for the initial condition, where the application prints it)
        assert r["steps"] == 2 and len(r["kinetic"]) == len(r["enstrophy"]) >= 2, (tag, r["stdout"][-1500:])
        assert len(r["kinetic"]) == len(runs["default"]["kinetic"]), (tag, r["stdout"][-1500:])
        assert len(r["state"]) == 4 * nv
        r["vel"], r["p"] = split(r["state"], nv, None if tag == "brick" else perm)
        assert np.abs(r["vel"]).max() > 0.5  # the lid moves
    # the paths announce themselves; the default path is today's general one and says nothing about boxes
    assert "box path: brick (gls_mesh_hyper_rectangle, 8 x 4 x 4 cells; multigrid attached)" in runs["brick"]["stderr"]
    assert "geometric multigrid V(1,1)-cycle on the nested hyper_rectangles (2 levels, coarsest 4 x 2 x 2 cells" \
        in runs["brick"]["stderr"]
    assert "box path" not in runs["default"]["stderr"] and "nested hyper_rectangles" not in runs["default"]["stderr"]
    d0 = differences(runs["ilu"], runs["jacobi"])
    d = differences(runs["brick"], runs["default"])
    print("app box path: d0 (default path, ilu vs jacobi) %s" % d0)
    print("app box path: brick vs default %s" % d)
    for key in d0:
        assert d[key] <= 4.0 * d0[key], (key, d[key], d0[key])


@pytest.mark.gpu
def test_odd_subdivision_falls_back_to_the_general_path(tmp_path):
    r = run(tmp_path, "odd", "--box-path", "brick", grid="3,1,1 : 0,0,0 : 3,1,1 : true", refinement=0)
    assert "box path: general (--box-path brick not taken: subdivisions * 2^refinement = 3 on axis 0 is not even)" \
        in r["stderr"], r["stderr"]
    assert "box path: brick" not in r["stderr"]
    assert r["steps"] == 2 and np.isfinite(r["state"]).all() and np.abs(r["state"]).max() > 0.5


@pytest.mark.gpu
def test_transient_kelly_falls_back_to_the_general_path(tmp_path):
    """mesh adaptation type kelly with the default `number mesh adapt = 0`: a transient run still adapts every
    `frequency` steps, so the box path is not taken (the fallback is announced, the run adapts at step 2 and finishes)"""
    r = run(tmp_path, "kelly", "--box-path", "brick", more=KELLY)
    assert "box path: general (--box-path brick not taken: Kelly mesh adaptation is not available on the box path)" \
        in r["stderr"], r["stderr"]
    assert "box path: brick" not in r["stderr"]
    assert r["steps"] == 2 and np.isfinite(r["state"]).all() and np.abs(r["state"]).max() > 0.5
    assert len(r["state"]) > 4 * int(np.prod([K * c + 1 for c in CELLS]))  # the mesh was refined
