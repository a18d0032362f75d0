"""--ic-eval device of the application: the L2projection initial condition by the library's device projection
(gls_projection_plan_create / gls_l2_projection) straight into the device-resident solution, instead of the host
conjugate gradients and an upload. The two initial states differ at rounding level (1e-14), so the runs print the
same lines with numbers that agree to 1e-9 relative; what the library does not serve (2D Q3) and --np take the host
path, say so on stderr, and print the host run's bytes."""
import os
import re
import subprocess

import pytest

from tests.test_gpu_app import tgv_prm
from tests.test_gpu_app_reference import CASES, ROOT

DEVICE, HOST = ("--ic-eval", "device"), ("--ic-eval", "host")
NUMBER = re.compile(r"[-+]?(?:\d+\.?\d*|\.\d+)(?:[eE][-+]?\d+)?")
SPLIT = re.compile(r"initial condition: L2 projection on the device \S+ s, (\d+) CG iterations, relative residual (\S+)")


def run_app(tmp_path, prm, dim, *extra):
    """(stdout, stderr) of one run with GLS_IC_SPLIT=1"""
    d = tmp_path / ("run%d" % len(list(tmp_path.iterdir())))
    d.mkdir()
    (d / "case.prm").write_text(prm)
    app = os.path.join(ROOT, "apps", "gls_navier_stokes_%dd" % dim)
    if not os.path.exists(app):
        pytest.fail("%s is not built (run __graft_entry__.build())" % app)
    out = subprocess.run([app, "--precision", "9", *extra, "case.prm"], cwd=str(d), capture_output=True, text=True,
                         timeout=600, env=dict(os.environ, GLS_IC_SPLIT="1"))
    assert out.returncode == 0, out.stderr[-3000:]
    return out.stdout, out.stderr


def same_lines_close_numbers(dev, host, rel=1e-9):
    """the same lines; every printed number equal to `rel` relative (compared as numbers, not as text)"""
    a, b = dev.splitlines(), host.splitlines()
    assert len(a) == len(b) > 0, (dev, host)
    n = 0
    for la, lb in zip(a, b):
        assert NUMBER.sub("#", la).split() == NUMBER.sub("#", lb).split(), (la, lb)
        for x, y in zip(NUMBER.findall(la), NUMBER.findall(lb)):
            x, y = float(x), float(y)
            assert abs(x - y) <= rel * max(abs(x), abs(y)), (la, lb)
            n += 1
    return n


def device_figures(stderr):
    m = SPLIT.search(stderr)
    assert m, stderr[-3000:]
    return int(m.group(1)), float(m.group(2))


@pytest.mark.gpu
def test_tgv_2d_periodic_sdirk2(tmp_path):
    """2D TGV, Q2-Q1, periodic, 16^2, two SDIRK2 steps, the error table, enstrophy and kinetic energy printed"""
    prm = tgv_prm("sdirk2", 2, 1, 4, 0.05, 0.1)
    dev, err = run_app(tmp_path, prm, 2, *DEVICE)
    host, herr = run_app(tmp_path, prm, 2, *HOST)
    assert "Kinetic energy" in dev and "L2 error velocity" in dev
    assert same_lines_close_numbers(dev, host) > 10
    its, res = device_figures(err)
    print("2D TGV: %d CG iterations, relative residual %.3e" % (its, res))
    assert 0 < its < 200 and res <= 1e-15
    assert "initial condition: on the device (gls_l2_projection)" in err
    assert "initial condition: L2 projection on the host" in herr and "on the device" not in herr


CUBE_3D = """
subsection simulation control
  set method           = bdf1
  set time step        = 0.05
  set time end         = 0.1
  set output frequency = 0
end
subsection physical properties
  set kinematic viscosity = 1.0
end
subsection mesh
  set type               = dealii
  set grid type          = hyper_cube
  set grid arguments     = -1 : 1 : false
  set initial refinement = 2
end
subsection FEM
  set velocity order = 2
  set pressure order = 1
end
subsection boundary conditions
  set number = 1
  subsection bc 0
    set type = function
    subsection u
      set Function expression = -y
    end
    subsection v
      set Function expression = x
    end
    subsection w
      set Function expression = 0
    end
  end
end
subsection initial conditions
  set type = L2projection
  subsection uvwp
    set Function expression = -y*cos(z); x*cos(z); 0.1*sin(x)*sin(y); sin(x) - 0.25*y*z
  end
end
subsection analytical solution
  set enable    = true
  set verbosity = verbose
  subsection uvw
    set Function expression = -y; x; 0; 0
  end
end
subsection post-processing
  set verbosity                = verbose
  set calculate enstrophy      = true
  set calculate kinetic energy = true
end
subsection non-linear solver
  set tolerance      = 1e-8
  set max iterations = 10
  set verbosity      = quiet
end
subsection linear solver
  set max iters         = 5000
  set relative residual = 1e-13
  set minimum residual  = 1e-14
end
"""


@pytest.mark.gpu
def test_cube_3d_function_boundary(tmp_path):
    """3D 4^3 Q2-Q1 with a non-zero `function` Dirichlet boundary held fixed by the projection, two BDF1 steps"""
    dev, err = run_app(tmp_path, CUBE_3D, 3, *DEVICE)
    host, _ = run_app(tmp_path, CUBE_3D, 3, *HOST)
    assert "Kinetic energy" in dev and "L2 error velocity" in dev
    assert same_lines_close_numbers(dev, host) > 10
    its, res = device_figures(err)
    print("3D cube: %d CG iterations, relative residual %.3e" % (its, res))
    assert 0 < its < 200 and res <= 1e-15


def mms2d(q3):
    """the reference's mms2d case on its first mesh, started from an L2-projected field"""
    prm = open(os.path.join(CASES, "mms2d_gls.prm")).read()
    prm = prm.replace("set number mesh adapt       = 2", "set number mesh adapt       = 0")
    prm += ("\nsubsection initial conditions\n  set type = L2projection\n  subsection uvwp\n"
            "    set Function expression = sin(pi*x)*y; cos(y)*x; sin(pi*x)+sin(pi*y)\n  end\nend\n")
    if q3:
        prm += "\nsubsection FEM\n  set velocity order = 3\n  set pressure order = 3\nend\n"
    return prm


@pytest.mark.gpu
def test_np2_uses_the_host_path(tmp_path):
    dev, err = run_app(tmp_path, mms2d(False), 2, "--np", "2", *DEVICE)
    host, _ = run_app(tmp_path, mms2d(False), 2, "--np", "2", *HOST)
    assert "initial condition: host projection (--np" in err
    assert "error_velocity" in dev and dev == host


@pytest.mark.gpu
def test_q3_falls_back_to_the_host_path(tmp_path):
    """2D Q3-Q3: gls_projection_plan_create answers GLS_EINVAL and the application projects on the host"""
    dev, err = run_app(tmp_path, mms2d(True), 2, *DEVICE)
    host, _ = run_app(tmp_path, mms2d(True), 2, *HOST)
    assert "initial condition: host projection (gls_projection_plan_create: FE_Q(3)" in err
    assert "error_velocity" in dev and dev == host
