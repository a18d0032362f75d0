"""Adaptive time stepping through the drop-in application (apps/gls_navier_stokes_{2d,3d}): 'simulation
control' entries adapt / max cfl / adaptative time step scaling / output control / output time, the step taken
from the library's controller (gls_time_control_*, the reference's SimulationControlTransient and
...DynamicOutput, source/core/simulation_control.cc:84-218) and the CFL from the one-pass device diagnostics
(gls_flow_diagnostics).

The log rule. A 'Transient iteration' line prints the iteration's time, its step and the CFL the controller
held when it chose that step: the CFL of the previous iteration's solution at the previous step (the
reference's print_progression prints get_CFL() after integrate()). So from line n-1's step and line n's CFL,
for n >= 2:  step_n = step_(n-1) * s,  s = max_cfl / CFL when CFL > 0 and max_cfl / CFL < scaling, else scaling;
then clamped to land on 'time end'. Line 1 keeps 'time step'. Checked to one unit in the sixth printed digit
(the log prints 6 significant digits).

The Taylor-Green case (2D, hyper_cube 0 : 2 pi refined 3 times = 8 x 8 cells, Q2-Q1, viscosity 1, time step 0.05):
with adapt = false the CFL printed on iterations 1, 2, 3 is 0.0975955, 0.0886259, 0.0802238 (the flow decays like
exp(-2 t)); max cfl = 0.1 lies between the first value and 1.2 times it, so the first steps grow by
max_cfl / CFL < 1.2 and, once the decay over a step exceeds 1.2, by the scaling: both branches within 8 steps."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests.test_gpu_app_configs import read_dumps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TGV = """
subsection simulation control
  set method                       = {method}
  set time step                    = 0.05
  set time end                     = {t_end}
  set adapt                        = {adapt}
  set max cfl                      = {max_cfl}
  set adaptative time step scaling = 1.2
  set output control               = {output_control}
  set output time                  = {output_time}
  set output name                  = tgv
  set output frequency             = {output_frequency}
end
subsection FEM
  set velocity order = 2
  set pressure order = 1
end
subsection initial conditions
  set type = L2projection
  subsection uvwp
    set Function expression = cos(x)*sin(y); -sin(x)*cos(y); -1./4*(cos(2*x)+cos(2*y));
  end
end
subsection physical properties
  set kinematic viscosity = 1.000
end
subsection post-processing
  set verbosity = verbose
  set calculate enstrophy = true
  set calculate kinetic energy = true
end
subsection mesh
  set type               = dealii
  set grid type          = hyper_cube
  set grid arguments     = 0 : 6.28318530718 : true
  set initial refinement = 3
end
subsection boundary conditions
  set number = 2
  subsection bc 0
    set type               = periodic
    set id                 = 0
    set periodic_id        = 1
    set periodic_direction = 0
  end
  subsection bc 1
    set type               = periodic
    set id                 = 2
    set periodic_id        = 3
    set periodic_direction = 1
  end
end
subsection non-linear solver
  set verbosity      = quiet
  set tolerance      = {tol}
  set max iterations = 10
end
subsection linear solver
  set verbosity                             = quiet
  set method                                = gmres
  set max iters                             = 5000
  set relative residual                     = 1e-10
  set minimum residual                      = 1e-13
  set ilu preconditioner fill               = 1
  set ilu preconditioner absolute tolerance = 1e-5
  set ilu preconditioner relative tolerance = 1.00
end
"""
TOL = 1e-8
SCALING, MAX_CFL = 1.2, 0.1


def tgv(method="bdf2", t_end=0.6, adapt="true", max_cfl=MAX_CFL, output_control="iteration", output_time=1,
        output_frequency=0):
    return TGV.format(method=method, t_end=t_end, adapt=adapt, max_cfl=max_cfl, output_control=output_control,
                      output_time=output_time, output_frequency=output_frequency, tol=TOL)


# the smallest mapped case of tests/golden/app_cases (taylorcouette_gls: hyper_shell, Q2-Q2, MappingQ2 on all
# cells) made transient: rigid rotation as the initial field, the inner cylinder turning, three adaptive steps
COUETTE = """
subsection simulation control
  set method                       = bdf1
  set time step                    = 0.02
  set time end                     = 0.07
  set adapt                        = true
  set max cfl                      = 0.12
  set adaptative time step scaling = 1.3
  set output frequency             = 0
end
subsection FEM
  set velocity order = 2
  set pressure order = 2
  set qmapping all   = true
end
subsection physical properties
  set kinematic viscosity = 1.0
end
subsection initial conditions
  set type = nodal
  subsection uvwp
    set Function expression = -y; x; 0
  end
end
subsection post-processing
  set verbosity = verbose
  set calculate enstrophy = true
  set calculate kinetic energy = true
end
subsection mesh
  set type               = dealii
  set grid type          = hyper_shell
  set grid arguments     = 0, 0 : 0.25 : 1 : 4:  true
  set initial refinement = 1
end
subsection boundary conditions
  set number = 2
  subsection bc 1
    set type = noslip
  end
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
subsection non-linear solver
  set tolerance      = 1e-8
  set max iterations = 10
  set verbosity      = quiet
end
subsection linear solver
  set method            = gmres
  set max iters         = 500
  set relative residual = 1e-6
  set minimum residual  = 1e-11
  set verbosity         = quiet
end
"""


def run(tmp_path, prm, dim=2, *extra):
    (tmp_path / "case.prm").write_text(prm)
    app = os.path.join(ROOT, "apps", "gls_navier_stokes_%dd" % dim)
    if not os.path.exists(app):
        pytest.fail("%s is not built (run __graft_entry__.build())" % app)
    r = subprocess.run([app, *extra, "case.prm"], cwd=str(tmp_path), capture_output=True, text=True, timeout=170)
    assert r.returncode == 0, r.stderr[-3000:] + "\nstdout tail:\n" + r.stdout[-2000:]
    return r.stdout


LINE = re.compile(r"^Transient iteration : (\d+)\s+Time : (\S+)\s+Time step : (\S+)\s+CFL : (\S+)")


def iterations(out):
    """[(iteration, time, step, cfl)] of the log"""
    rows = [LINE.match(l) for l in out.splitlines()]
    rows = [(int(m.group(1)), float(m.group(2)), float(m.group(3)), float(m.group(4))) for m in rows if m]
    assert [r[0] for r in rows] == list(range(1, len(rows) + 1)), rows
    return rows


def unit6(v):
    """one unit in the sixth significant digit of v as the log prints it"""
    return 10.0 ** (math.floor(math.log10(abs(v))) - 5)


def check_log_rule(rows, dt0, t_end, max_cfl, scaling):
    """the rule of the module docstring on every line; returns the branch taken per iteration"""
    branches = []
    for i, (n, time, dt, cfl) in enumerate(rows):
        t_prev = rows[i - 1][1] if i else 0.0
        if n == 1:
            want, branch = dt0, "first"
        else:
            prev = rows[i - 1][2]
            if cfl > 0 and max_cfl / cfl < scaling:
                want, branch = prev * max_cfl / cfl, "cfl"
            else:
                want, branch = prev * scaling, "scaling"
        tol = unit6(dt)
        if t_prev + want > t_end:
            # a difference of printed numbers: half a unit of the printed time's last digit and half a unit of
            # the printed step's (the time has the coarser last digit)
            want, branch = t_end - t_prev, "clamp"
            tol = 0.5 * (unit6(t_prev) + unit6(dt))
        print("iteration %d: time %g step %g (rule: %.7g, %s) CFL %g" % (n, time, dt, want, branch, cfl))
        assert abs(dt - want) <= tol * (1 + 1e-9), (n, dt, want, branch)
        # a sum of printed numbers: half a unit of each one's last digit
        t_tol = 0.5 * (unit6(time) + unit6(dt) + (unit6(t_prev) if i else 0.0))
        assert abs(time - (t_prev + dt)) <= t_tol * (1 + 1e-9), (n, time, t_prev, dt)
        branches.append(branch)
    assert rows[-1][1] == t_end, rows[-1]
    return branches


@pytest.mark.gpu
def test_tgv_bdf2_adaptive_steps_and_oracle_replay(tmp_path):
    from oracle.oracle import Oracle, StructuredProblem
    dump = tmp_path / "dump"
    dump.mkdir()
    out = run(tmp_path, tgv(), 2, "--dump", str(dump))
    rows = iterations(out)
    branches = check_log_rule(rows, 0.05, 0.6, MAX_CFL, SCALING)
    assert len(rows) <= 10 and "cfl" in branches and "scaling" in branches and branches[-1] == "clamp", branches
    # every iterate solves the reference's discrete equations with the steps the log shows: the oracle's
    # residual at the dumped state, with the dump's scheme and time steps, is below the Newton tolerance
    # (margin 1.01 as tests/test_gpu_app_configs.py)
    dumps = read_dumps(str(dump))
    assert len(dumps) == len(rows)
    for (n, time, dt, cfl), d in zip(rows, dumps):
        assert int(d["step"]) == n and int(d["scheme"]) == 2  # GLS_BDF2
        ts = d["time_steps"]
        if n == 1:  # the start-up: a BDF1 sub-step of 0.4 dt, then BDF2 over the rest
            assert abs(ts[0] + ts[1] - dt) <= unit6(dt)
        else:
            assert abs(ts[0] - dt) <= 0.5 * unit6(dt) * (1 + 1e-9), (n, ts, dt)
            if n > 2:
                assert abs(ts[1] - rows[n - 2][2]) <= 0.5 * unit6(ts[1]) * (1 + 1e-9), (n, ts)
        p = StructuredProblem(2, 8, k=2, kp=1, lo=0.0, hi=6.28318530718, colorize=True, viscosity=1.0, scheme="bdf2",
                              time_steps=tuple(ts), periodic=(0, 1))
        assert int(d["n_dofs"]) == p.n_dofs
        res = np.linalg.norm(Oracle(p).residual(d["x"], d["m1"], d["m2"], d["m3"]))
        print("iteration %d: oracle residual %.3e with time steps %s" % (n, res, ts[:2]))
        assert res <= 1.01 * TOL, (n, res)


@pytest.mark.gpu
@pytest.mark.parametrize("method", ["bdf3", "sdirk2"])
def test_tgv_other_schemes_follow_the_rule(tmp_path, method):
    """four steps: the first keeps the step, the next two follow the CFL, the last is clamped"""
    rows = iterations(run(tmp_path, tgv(method=method, t_end=0.22)))
    assert len(rows) == 4, rows
    branches = check_log_rule(rows, 0.05, 0.22, MAX_CFL, SCALING)
    assert branches[0] == "first" and branches[-1] == "clamp", branches


@pytest.mark.gpu
def test_output_control_time(tmp_path):
    """output time 0.13 is no multiple of any step: the controller forces a step onto each multiple, the .pvd lists
    exactly those (the reference's DynamicOutput writes nothing at t = 0: its first output time is 0.13), and the
    step after a forced one is the step before it again"""
    out = run(tmp_path, tgv(t_end=0.45, output_control="time", output_time=0.13, output_frequency=1))
    rows = iterations(out)
    assert rows[-1][1] == 0.45
    pvd = (tmp_path / "tgv.pvd").read_text()
    times = [float(t) for t in re.findall(r'timestep="([^"]+)"', pvd)]
    assert len(times) == 3 and np.abs(np.array(times) - 0.13 * np.arange(1, 4)).max() <= 1e-12, times
    forced = [i for i, r in enumerate(rows) if min(abs(r[1] - t) for t in times) <= unit6(r[1])]
    assert len(forced) == 3, (rows, times)
    for i in forced:
        assert rows[i][2] < rows[i - 1][2] * 0.999, rows[i]  # cut short to land on the output time
        if i + 1 < len(rows) - 1:  # (the last step is clamped to the end)
            assert rows[i + 1][2] == rows[i - 1][2], (rows[i - 1], rows[i], rows[i + 1])


@pytest.mark.gpu
def test_unknown_output_control_is_an_error(tmp_path):
    (tmp_path / "case.prm").write_text(tgv(output_control="sometimes"))
    r = subprocess.run([os.path.join(ROOT, "apps", "gls_navier_stokes_2d"), "case.prm"], cwd=str(tmp_path),
                       capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "output control" in r.stderr + r.stdout


def pp_values(out, key):
    return [float(l.split(":")[1]) for l in out.splitlines() if l.startswith(key)]


@pytest.fixture(scope="module")
def couette_one_rank(tmp_path_factory):
    return run(tmp_path_factory.mktemp("couette1"), COUETTE)


@pytest.mark.gpu
def test_general_mesh_adaptive_steps(couette_one_rank):
    """mapped Q2 cells: CFL, kinetic energy and enstrophy from the device pass; three steps obey the rule"""
    out = couette_one_rank
    rows = iterations(out)
    assert len(rows) == 3, rows
    check_log_rule(rows, 0.02, 0.07, 0.12, 1.3)
    assert rows[0][3] > 0
    ke, en = pp_values(out, "Kinetic energy"), pp_values(out, "Enstrophy")
    assert len(ke) == 4 and len(en) == 4 and min(ke) > 0 and min(en) > 0, (ke, en)


@pytest.mark.gpu
def test_two_ranks_agree_with_one(tmp_path, couette_one_rank):
    """--np 2: every rank's pass over its own cells, the four numbers combined (maximum / sums in rank order).
    The step-0 enstrophy and kinetic energy and the CFL printed on iteration 1 depend on the initial condition
    only: equal to one rank's to one unit in the sixth printed digit (the summation order differs)"""
    out2 = run(tmp_path, COUETTE, 2, "--np", "2")
    assert "Running on 2 MPI rank(s)" in out2
    for key in ("Enstrophy", "Kinetic energy"):
        a, b = pp_values(couette_one_rank, key)[0], pp_values(out2, key)[0]
        assert abs(a - b) <= unit6(a) * (1 + 1e-9), (key, a, b)
    a, b = iterations(couette_one_rank)[0][3], iterations(out2)[0][3]
    assert a > 0 and abs(a - b) <= unit6(a) * (1 + 1e-9), (a, b)
