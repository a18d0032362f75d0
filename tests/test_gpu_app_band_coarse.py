"""GPU: the application's --coarse-storage option. The (1, "hmg") case of
test_configs4_cylinder3d_re200_bdf2_kelly_pipeline (Re 200 past the 1-layer extruded cylinder, Q2-Q1, BDF, the
hierarchy multigrid with the Q1-Q1 p-level on the base mesh) cut to one time step, with the p-level's LU in band
storage (--coarse-storage band) and in the dense arrays (dense): the band run announces `banded LU`, solves the
reference's discrete equations (the oracle's residual at its dump) and takes the dense run's linear iterations to
within one per Newton step."""
import os
import re

import numpy as np
import pytest

from tests.test_gpu_app_configs import CASES, MESHES, SCHEME_NAMES, problem, run_app, setprm

TOL = 1e-8


def one_step(tmp_path, storage):
    prm = open(os.path.join(CASES, "cylinder3d_q2q1_re200_kelly.prm")).read()
    prm = setprm(prm, "file name", "cylinder3d_1layer.msh")
    prm = setprm(prm, "time end", "0.05")
    prm = setprm(prm, "tolerance", "%g" % TOL)
    prm = setprm(prm, "relative residual", "1e-10")
    prm = setprm(prm, "minimum residual", "1e-13")
    d = tmp_path / storage
    d.mkdir()
    out, dumps = run_app(d, prm, [os.path.join(MESHES, "cylinder3d_1layer.msh")],
                         extra=("--np", "1", "--precond", "hmg", "--coarse-storage", storage))
    m = re.search(r"newton_iterations = (\d+), linear_iterations = (\d+)", out)
    assert m, out[-1500:]
    steps = [int(x) for x in re.findall(r"-Iterative solver took : (\d+) steps", out)]  # one per Newton step
    assert sum(steps) == int(m.group(2)), (steps, m.group(0))
    return out, dumps, (d / "stderr.txt").read_text(), int(m.group(1)), steps


@pytest.mark.gpu
def test_band_coarse_storage_one_step(tmp_path):
    from oracle.oracle import Oracle
    from softx_2020_200_amd.native import UMesh
    out, dumps, err, newton, linear = one_step(tmp_path, "band")
    _, dumps_d, err_d, newton_d, linear_d = one_step(tmp_path, "dense")
    line = [l for l in err.splitlines() if "banded LU" in l]
    print("band: newton %d linear %s; dense: newton %d linear %s\n%s" % (newton, linear, newton_d, linear_d, line))
    assert len(dumps) == 1 and len(dumps_d) == 1, out
    assert line and re.search(r"Q1-Q1 p-level on the base mesh, banded LU \(n \d+, bandwidths \d+/\d+, [0-9.]+ GB\)", line[0]), \
        err[-1500:]
    assert "banded LU" not in err_d and "Q1-Q1 p-level on the base mesh, dense LU" in err_d, err_d[-1500:]
    m = UMesh(3, gmsh=os.path.join(MESHES, "cylinder3d_1layer.msh"))
    inlet = lambda X: np.stack([np.ones(len(X)), 0 * X[:, 0], 0 * X[:, 0]], 1)
    bcs = [("noslip", 0, None), ("function", 1, inlet), ("slip", 2, None), ("slip", 4, None), ("slip", 5, None)]
    sp = m.fe_space_handle(2, 1).data
    d = dumps[0]
    assert int(d["n_cells"]) == sp["n_cells"] and int(d["n_dofs"]) == 3 * sp["n_vnodes"] + sp["n_pnodes"]
    p = problem(sp, 0.005, bcs, SCHEME_NAMES[int(d["scheme"])], d["time_steps"])
    res = np.linalg.norm(Oracle(p).residual(d["x"], d["m1"], d["m2"], d["m3"]))
    print("oracle residual at the band run's dump: %.3e (tol %.1e)" % (res, TOL))
    assert res <= 1.01 * TOL, res
    # the linear iterations of every Newton step within 1 of the dense run's
    assert newton == newton_d and len(linear) == len(linear_d), (newton, linear, newton_d, linear_d)
    assert all(abs(a - b) <= 1 for a, b in zip(linear, linear_d)), (linear, linear_d)


def test_unknown_coarse_storage_is_refused(tmp_path):  # (the options are parsed before anything touches a GPU)
    import subprocess
    from tests.test_gpu_app_configs import ROOT
    app = os.path.join(ROOT, "apps", "gls_navier_stokes_3d")
    assert os.path.exists(app), "apps/gls_navier_stokes_3d is not built (run __graft_entry__.build())"
    r = subprocess.run([app, "--coarse-storage", "banana", "case.prm"], cwd=str(tmp_path), capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 1 and "--coarse-storage banana: auto, dense or band" in r.stderr, (r.returncode, r.stderr)
