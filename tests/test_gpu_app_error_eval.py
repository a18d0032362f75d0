"""--error-eval device of the application: the L2 error against the analytical solution from the device-resident
solution (gls_error_plan_create / gls_l2_error) instead of the host pass over a downloaded vector. The reference's
cases reproduce their golden .output with it exactly as tests/test_gpu_app_reference.py checks them with the host
path, the stdout of the two paths is equal line for line, and what the library has no kernel for (2D Q3) and
--np fall back to the host path with unchanged output."""
import os
import re
import subprocess

import pytest

from tests.test_gpu_app_reference import CASES, ROOT, error_rows, run_case, setup_lines

DEVICE, HOST = ("--error-eval", "device"), ("--error-eval", "host")
# name -> (dim, the pressure column is compared exactly)
STEADY = {"mms2d_gls": (2, True), "taylorcouette_gls": (2, False), "mms2d-unstructured_gls": (2, True)}
TGV = "taylor-green-vortex_gls_sdirk2"
_runs = {}


def no_output(prm):
    return re.sub(r"set output frequency\s*=\s*1 ", "set output frequency = 1000000 ", prm)


def run(tmp_path_factory, name, dim, extra, prm_edit=None, tag=""):
    """the stdout of one run, shared by the tests that read it"""
    key = (name, extra, tag)
    if key not in _runs:
        _runs[key] = run_case(tmp_path_factory.mktemp("run"), name, dim, *extra, prm_edit=prm_edit)
    return _runs[key]


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(STEADY))
def test_reference_case_with_the_device_error(tmp_path_factory, name):
    dim, pressure = STEADY[name]
    ref = open(os.path.join(CASES, name + ".output")).read()
    out = run(tmp_path_factory, name, dim, DEVICE)
    assert setup_lines(out) == setup_lines(ref), out
    ro, rr = error_rows(out), error_rows(ref)
    print(name, "ours", ro, "reference", rr)
    assert len(ro) == len(rr) > 0, out
    for a, b in zip(ro, rr):
        assert a[0] == b[0]  # cells
        assert a[1] == b[1], (name, a, b)  # error_velocity at the printed digits
        if len(b) > 2 and b[2] != "-":
            assert a[2] == b[2], (name, a, b)
        if pressure:
            assert a[3:] == b[3:], (name, a, b)
        else:  # taylorcouette_gls: the reference's column carries its solver's free pressure constant
            assert float(a[3]) < float(b[3]), (name, a, b)


@pytest.mark.gpu
def test_reference_tgv_sdirk2_with_the_device_error(tmp_path_factory):
    """time-dependent and verbose: the error at the time of the step"""
    ref = open(os.path.join(CASES, TGV + ".output")).read()
    out = run(tmp_path_factory, TGV, 2, DEVICE, prm_edit=no_output)
    pick = lambda t, key: [l.split(":")[1].strip() for l in t.splitlines() if l.startswith(key)]  # noqa: E731
    for key in ("Enstrophy", "Kinetic energy"):
        assert pick(out, key) == pick(ref, key), (key, pick(out, key), pick(ref, key))
    e, r = float(pick(out, "L2 error velocity")[0]), float(pick(ref, "L2 error velocity")[0])
    assert abs(e - r) <= 1e-5 * r, (e, r)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(STEADY) + [TGV])
def test_host_and_device_print_the_same(tmp_path_factory, name):
    dim = STEADY.get(name, (2, None))[0]
    edit = no_output if name == TGV else None
    dev = run(tmp_path_factory, name, dim, DEVICE, prm_edit=edit)
    host = run(tmp_path_factory, name, dim, HOST, prm_edit=edit)
    assert "error" in dev.lower() and dev.splitlines() == host.splitlines()


def q3(prm):
    return prm.replace("set number mesh adapt       = 2", "set number mesh adapt       = 1") + (
        "\nsubsection FEM\n  set velocity order = 3\n  set pressure order = 3\nend\n")


@pytest.mark.gpu
@pytest.mark.parametrize("edit,note,count", [(None, "L2 error: on the device (gls_l2_error)", 3),
                                             (q3, "L2 error: host evaluation (gls_error_plan_create: FE_Q(3)", 2)],
                         ids=["q1", "q3"])
def test_which_path_ran_is_announced_on_stderr(tmp_path, edit, note, count):
    """equal output does not show which path produced it: the application says so on stderr, once per mesh (a plan is
    made, or refused, after every refinement)"""
    prm = open(os.path.join(CASES, "mms2d_gls.prm")).read()
    (tmp_path / "case.prm").write_text(edit(prm) if edit else prm)
    app = os.path.join(ROOT, "apps", "gls_navier_stokes_2d")
    run_ = lambda *extra: subprocess.run([app, *extra, "case.prm"], cwd=str(tmp_path), capture_output=True, text=True,  # noqa: E731
                                         timeout=600)
    out = run_(*DEVICE)
    assert out.returncode == 0, out.stderr[-3000:]
    assert sum(l.startswith(note) for l in out.stderr.splitlines()) == count, out.stderr[-3000:]
    assert "L2 error:" not in run_().stderr  # the default is the host path, silently


@pytest.mark.gpu
def test_q3_falls_back_to_the_host_path(tmp_path_factory):
    """2D Q3-Q3: gls_error_plan_create answers GLS_EINVAL and the application evaluates on the host"""
    dev = run(tmp_path_factory, "mms2d_gls", 2, DEVICE, prm_edit=q3, tag="q3")
    host = run(tmp_path_factory, "mms2d_gls", 2, HOST, prm_edit=q3, tag="q3")
    assert len(error_rows(dev)) == 2 and dev.splitlines() == host.splitlines()


@pytest.mark.gpu
def test_np2_uses_the_host_path(tmp_path_factory):
    dev = run(tmp_path_factory, "mms2d_gls", 2, ("--np", "2") + DEVICE)
    host = run(tmp_path_factory, "mms2d_gls", 2, ("--np", "2"))
    assert len(error_rows(dev)) == 3 and dev.splitlines() == host.splitlines()
