"""The reference's force / torque post-processing through the drop-in binaries (the `forces` prm section,
navier_stokes_base.cc:120-250, 855-881, 1088-1121): the 'Force  summary' / 'Torque summary' tables of the
reference's .output files (tests/golden/app_cases/) and the <name>.<NN>.dat files. This lifts the exception
documented in tests/test_gpu_app_reference.py ("the torque summary (forces are out of scope) is not
produced"): the tables are produced and compared here. Tables are parsed into numbers; whitespace is not
compared (the golden files are ragged: several ranks' streams interleave there)."""
import glob
import os
import re
import subprocess

import pytest

from tests.test_gpu_app_reference import CASES, ROOT, run_case

CONVERGED = lambda t: t.replace("set tolerance               = 1e-4", "set tolerance = 1e-10").replace(  # noqa: E731
    "set relative residual       = 1e-4", "set relative residual = 1e-12").replace(
    "set minimum residual        = 1e-9", "set minimum residual = 1e-14")


# cylinder_gls: measured max |f - f_golden| / max |f_golden| of the four tables (see
# test_reference_cylinder_force_tables)
MEASURED = [1.409e-07, 1.419e-07, 2.245e-05, 3.299e-05]


def summaries(text, kind):
    """[(ids, rows of value strings)] of every '<kind> summary' table in a log"""
    lines = text.splitlines()
    out = []
    for i, l in enumerate(lines):
        if not re.match(r"\|\s+%s\s+summary" % kind, l):
            continue
        assert lines[i + 2].split()[:2] == ["Boundary", "ID"], lines[i + 2]
        ids, rows = [], []
        for r in lines[i + 3:]:
            t = r.split()
            if not t or not re.fullmatch(r"\d+", t[0]) or not all(re.fullmatch(r"-?\d+\.\d+", v) for v in t[1:]):
                break
            ids.append(int(t[0]))
            rows.append(t[1:])
        out.append((ids, rows))
    return out


def digits(s):
    return len(s.split(".")[1])


def read_dat(path):
    rows = [l.split() for l in open(path).read().splitlines() if l.strip()]
    assert rows[0][0] == "time", rows[0]
    return [[float(v) for v in r] for r in rows[1:]]


@pytest.mark.gpu
@pytest.mark.parametrize("name,dim,n_bc", [("taylorcouette_gls", 2, 2), ("rigid-body-rotation_gls", 2, 2),
                                          ("cylinder-rigid-body_gls", 3, 1)])
def test_reference_torque_tables(tmp_path, name, dim, n_bc):
    """Every Torque summary of the golden .output appears with the same boundary ids; each value within one
    unit of the last printed digit (the solves are inexact by the prm: the allowance of the existing
    poiseuille_gls check); torque.NN.dat: one row per iteration, 4 columns, equal to the log at its digits."""
    ref = summaries(open(os.path.join(CASES, name + ".output")).read(), "Torque")
    out = summaries(run_case(tmp_path, name, dim), "Torque")
    print(name, "ours", out, "reference", ref)
    assert len(ref) >= 2 and len(out) == len(ref)
    for (ia, ra), (ib, rb) in zip(out, ref):
        assert ia == ib and len(ia) == n_bc
        for a, b in zip(ra, rb):
            assert len(a) == len(b) == 3
            for va, vb in zip(a, b):
                assert digits(va) == digits(vb)
                assert abs(float(va) - float(vb)) <= 1.0000001 * 10.0 ** -digits(vb), (va, vb)
    files = sorted(os.path.basename(f) for f in glob.glob(str(tmp_path / "torque.*.dat")))
    assert files == ["torque.%02d.dat" % i for i in range(n_bc)]
    assert not glob.glob(str(tmp_path / "force.*.dat"))
    for i in range(n_bc):
        rows = read_dat(tmp_path / ("torque.%02d.dat" % i))
        assert len(rows) == len(out) and all(len(r) == 4 for r in rows)
        for it, r in enumerate(rows):
            assert r[0] == it + 1  # steady: the iteration number
            for v, printed in zip(r[1:], out[it][1][i]):
                assert abs(v - float(printed)) <= 0.5000001 * 10.0 ** -digits(printed), (v, printed)


@pytest.mark.gpu
def test_reference_cylinder_force_tables(tmp_path):
    """cylinder_gls with the converged-solve prm edit of test_reference_cylinder_kelly_adaptation_converged
    (all four meshes equal the reference's): four 'Force  summary' tables with ids 0, 1, 2. The golden
    forces came from the reference's inexact solves (Newton tolerance 1e-4), so the bound on
    max |f - f_golden| / max |f_golden| per table is measured: 1.409e-07, 1.419e-07, 2.245e-05, 3.299e-05
    (MEASURED; the first two meshes' solves agree to the printed digits, the adapted ones to 3e-5).
    The assertion is 3x the largest of them, which must stay <= 1e-3 (ten times that Newton tolerance); a
    sign error, a missing transpose term or a wrong face rule is far outside it. force.00.dat ..
    force.02.dat hold 4 rows each."""
    ref = summaries(open(os.path.join(CASES, "cylinder_gls.output")).read(), "Force")
    out = summaries(run_case(tmp_path, "cylinder_gls", 2, prm_edit=CONVERGED), "Force")
    assert len(ref) == 4 and len(out) == 4
    measured = []
    for (ia, ra), (ib, rb) in zip(out, ref):
        assert ia == ib == [0, 1, 2]
        fa = [float(v) for r in ra for v in r]
        fb = [float(v) for r in rb for v in r]
        assert len(fa) == len(fb) == 6
        measured.append(max(abs(a - b) for a, b in zip(fa, fb)) / max(abs(b) for b in fb))
    print("cylinder_gls: max |f - f_golden| / max |f_golden| per table:", ["%.3e" % v for v in measured])
    bound = 3 * max(MEASURED)
    assert bound <= 1e-3
    assert max(measured) <= bound, measured
    for i in range(3):
        rows = read_dat(tmp_path / ("force.%02d.dat" % i))
        assert len(rows) == 4 and all(len(r) == 4 for r in rows)
        assert [r[0] for r in rows] == [1, 2, 3, 4] and all(r[3] == 0.0 for r in rows)  # f_z = 0 in 2D


@pytest.mark.gpu
def test_two_ranks_print_the_same_tables(tmp_path):
    """--np 2: rank 0 evaluates on the gathered solution over the whole mesh; the parsed tables equal the
    one-rank run's"""
    one, two = tmp_path / "one", tmp_path / "two"
    one.mkdir()
    two.mkdir()
    a = summaries(run_case(one, "taylorcouette_gls", 2), "Torque")
    b = summaries(run_case(two, "taylorcouette_gls", 2, "--np", "2"), "Torque")
    print("one rank", a, "two ranks", b)
    assert len(a) == 3
    assert [(i, [[float(v) for v in r] for r in rows]) for i, rows in a] == \
        [(i, [[float(v) for v in r] for r in rows]) for i, rows in b]


@pytest.mark.gpu
def test_mixed_switches(tmp_path):
    """forces and torques on, verbosity quiet, calculation / output frequency 2 on the 3-iteration steady
    taylorcouette_gls: no table on the log, the files hold the rows of the even steps only"""
    def edit(t):
        for key, val in (("verbosity", "quiet"), ("calculate forces", "true"), ("calculation frequency", "2"),
                         ("output frequency", "2")):
            t, n = re.subn(r"(subsection forces.*?set %s\s*=\s*)\w+" % key, r"\g<1>" + val, t, flags=re.S)
            assert n == 1, key
        return t
    out = run_case(tmp_path, "taylorcouette_gls", 2, prm_edit=edit)
    assert "summary" not in out
    for stem in ("force", "torque"):
        for i in range(2):
            rows = read_dat(tmp_path / ("%s.%02d.dat" % (stem, i)))
            assert [r[0] for r in rows] == [2.0] and len(rows[0]) == 4, (stem, i, rows)
    t1 = read_dat(tmp_path / "torque.01.dat")[0]
    assert abs(t1[3] - 0.836) < 2e-3  # the second iteration's T_z of the golden table


@pytest.mark.gpu
def test_defaults_print_and_write_nothing(tmp_path):
    """no forces section (mms2d_gls): no summary box on the log, no force / torque .dat (the error table's
    L2Error.dat is the only .dat, as before)"""
    assert "subsection forces" not in open(os.path.join(CASES, "mms2d_gls.prm")).read()
    out = run_case(tmp_path, "mms2d_gls", 2)
    assert "summary" not in out
    assert sorted(os.path.basename(f) for f in glob.glob(str(tmp_path / "*.dat"))) == ["L2Error.dat"]


@pytest.mark.gpu
def test_degrees_without_a_load_kernel_die_with_the_limit(tmp_path):
    """2D Q3-Q3 with forces on: the library's GLS_EINVAL becomes a die at setup that names the limit"""
    prm = open(os.path.join(CASES, "mms2d_gls.prm")).read()
    assert "subsection FEM" not in prm and "subsection forces" not in prm
    prm += "\nsubsection FEM\n  set velocity order = 3\n  set pressure order = 3\nend\n"
    prm += "subsection forces\n  set calculate forces = true\nend\n"
    (tmp_path / "case.prm").write_text(prm)
    out = subprocess.run([os.path.join(ROOT, "apps", "gls_navier_stokes_2d"), "case.prm"], cwd=str(tmp_path),
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 1 and "2D Q3 is not supported" in out.stderr, out.stderr[-2000:]
    assert "summary" not in out.stdout
