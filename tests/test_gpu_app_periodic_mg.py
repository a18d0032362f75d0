"""GPU: apps/gls_navier_stokes on the periodic Taylor-Green box (apps/cases/tgv3d_q2q2_bdf2.prm) with the periodic nested
multigrid it now attaches by default, against its ILU path on the same case; and the steady, fully periodic problem,
which keeps the ILU path.

The tolerance of the comparison is measured, not chosen: D0 is the difference the two solvers the application had before
(--precond ilu and --precond jacobi) show on this very case (refinement 4, three BDF2 steps, Newton tolerance 1e-9,
linear relative residual 1e-8), per quantity; the multigrid run may differ from the ILU run by 4 D0."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(ROOT, "apps", "gls_navier_stokes")
CASE = os.path.join(ROOT, "apps", "cases", "tgv3d_q2q2_bdf2.prm")

# max |ilu - jacobi| over the three steps' tables and over the final state (velocity DoFs; pressure DoFs with the
# mean taken out: the periodic box fixes the pressure up to a constant), measured on an MI355X
# (the tables print six significant digits, on which the two agree to the last one)
D0 = {"kinetic": 0.0, "enstrophy": 0.0, "velocity": 6.348116476928567e-13, "pressure": 1.678387984149765e-11}


def setprm(text, key, value):
    new, n = re.subn(r"(set %s\s*=\s*)[^\n#]*" % re.escape(key), r"\g<1>%s" % value, text)
    assert n >= 1, key
    return new


def case_prm(steps=3):
    t = open(CASE).read()
    t = setprm(t, "initial refinement", 4)
    t = setprm(t, "time end", 0.05 * steps)
    t = setprm(t, "tolerance", "1e-9")
    t = setprm(t, "relative residual", "1e-8")
    t = setprm(t, "minimum residual", "1e-14")
    return t.replace("set type = end", "set type = none")


def run(tmp_path, tag, prm, *extra):
    d = tmp_path / tag
    d.mkdir()
    (d / "case.prm").write_text(prm)
    (d / "dump").mkdir()
    if not os.path.exists(APP):
        pytest.fail("apps/gls_navier_stokes is not built (run __graft_entry__.build())")
    out = subprocess.run([APP, "--dim", "3", "--precision", "12", "--stats", "--dump", str(d / "dump"), *extra, "case.prm"],
                         cwd=str(d), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:] + out.stdout[-2000:]
    vals = lambda key: np.array([float(l.split(":")[1]) for l in out.stdout.splitlines() if l.startswith(key)])
    its = [int(l.split("linear_iterations =")[1]) for l in out.stdout.splitlines() if "linear_iterations =" in l]
    last = sorted(f for f in os.listdir(d / "dump") if f.endswith(".bin"))[-1]
    meta = dict(l.split(" ", 1) for l in open(d / "dump" / last.replace(".bin", ".meta")).read().splitlines())
    n = int(meta["n_dofs"])
    state = np.fromfile(d / "dump" / last, dtype=np.float64)[:n]
    return dict(kinetic=vals("Kinetic energy :"), enstrophy=vals("Enstrophy  :"), state=state, its=its[-1],
                stderr=out.stderr, stdout=out.stdout)


def differences(a, b):
    nv = 3 * (len(a["state"]) // 4)
    pa, pb = a["state"][nv:] - a["state"][nv:].mean(), b["state"][nv:] - b["state"][nv:].mean()
    assert len(a["kinetic"]) == len(b["kinetic"]) >= 3 and len(a["enstrophy"]) == len(b["enstrophy"]) >= 3
    return dict(kinetic=float(np.abs(a["kinetic"] - b["kinetic"]).max()),
                enstrophy=float(np.abs(a["enstrophy"] - b["enstrophy"]).max()),
                velocity=float(np.abs(a["state"][:nv] - b["state"][:nv]).max()), pressure=float(np.abs(pa - pb).max()))


@pytest.mark.gpu
def test_app_periodic_multigrid_same_physics_as_ilu(tmp_path):
    prm = case_prm()
    mg = run(tmp_path, "mg", prm)
    ilu = run(tmp_path, "ilu", prm, "--precond", "ilu")
    assert "periodic geometric multigrid" in mg["stderr"] and "gls_mg_attach_periodic" not in mg["stderr"], mg["stderr"][-800:]
    assert "multigrid" not in ilu["stderr"] and "ILU(" in ilu["stderr"], ilu["stderr"][-800:]
    d = differences(mg, ilu)
    print("periodic app: multigrid vs ILU differences %s (D0 %s), linear iterations %d vs %d" % (d, D0, mg["its"], ilu["its"]))
    # the state is the Taylor-Green vortex: kinetic energy 1/8 and enstrophy 3/8 of the 3D field at t = 0, nearly kept
    assert abs(ilu["kinetic"][0] - 0.125) < 2e-3 and abs(ilu["enstrophy"][0] - 0.375) < 2e-2, (ilu["kinetic"], ilu["enstrophy"])
    for key, v in d.items():
        assert v <= 4.0 * D0[key], (key, v, D0[key])
    assert mg["its"] < ilu["its"], (mg["its"], ilu["its"])


@pytest.mark.gpu
def test_app_steady_fully_periodic_keeps_the_ilu_path(tmp_path):
    """steady and fully periodic: the constant velocity is in the null space of every level, no hierarchy is attached;
    the linear solver announcement is the ILU's, word for word what it was, and the run finishes"""
    prm = case_prm().replace("set method           = bdf2", "set method           = steady")
    assert "= steady" in prm
    prm = setprm(prm, "initial refinement", 3)
    prm = setprm(prm, "kinematic viscosity", "1.0")
    prm = setprm(prm, "max iterations", "3")
    r = run(tmp_path, "steady", prm)
    lines = [l for l in r["stderr"].splitlines() if l.startswith("linear solver:")]
    assert lines == ["linear solver: method = gmres -> GMRES + ILU(0) atol 1e-08 rtol 1"], r["stderr"][-800:]
    assert "multigrid: not attached on a steady, fully periodic box" in r["stderr"]
    assert np.isfinite(r["state"]).all()
