"""The application's VTU output evaluated on the device (--output-eval device, the default on one rank) against the
host evaluation it replaces (--output-eval host): the same log, the same files, byte-equal pvtu / pvd records,
and in every .vtu piece byte-equal connectivity / offsets / types / subdomain arrays and point data within the
project's 1e-12 device-versus-restatement tolerance (tests/test_gpu_output_fields.py). Here only the files
exist, so the scales come from the host run's arrays:
  velocity, pressure     their own maximum
  points                 the domain extent (box cells: the points are equal)
  vorticity              max |omega| / 2 <= max |grad u|: not wider than the scale of the field test
  q_criterion at p       0.5 sum_{p' <= p} (|W|^2 + |S|^2) = 0.5 sum_{p' <= p} |omega|^2 - q_p exactly, since
                         |W|^2 = |omega|^2 / 2 and sum |S|^2 = sum |W|^2 - 2 q_p
On the TGV case every point of every piece is held to these scales as they stand.

The cylinder's flow is smooth: far from the wall |grad u| is 1e-5 of its maximum, and in the first file (the uniform
initial field on mapped cells) it is zero -- there the host's dense sum leaves rounding noise (|grad u| ~ 1e-15,
q ~ 1e-30) where the sum-factorized sweeps give exact zeros. The rounding error of a gradient is absolute, whatever
|grad u| is, so at such points the host's own q is not accurate to 1e-12 of the cell's scale and no second order of
summation can agree with it to that (measured error over the per-cell scale: 1.0 in the first file, 9.3e-10 and
1.7e-9 in the others). The cylinder pieces are therefore split by a criterion computed from the host file alone:
  delta_c = 3 * 8 * dim * eps * max|u|_cell / hmin_cell   the first-order rounding bound of one gradient entry: sums
            of 3 terms per direction, sum |D_a| = 8 for the Q2 derivative row at an end point, dim reference
            directions through J^-1, 1 / h from the patch's shortest edge; two evaluations differ by 2 delta_c
            per entry, dim * 2 delta_c in the Frobenius norm
  B_p     = sum_{p' <= p} (2 |G_p'|_F dim 2 delta_c + (dim 2 delta_c)^2), |G_p'|_F^2 = 2 (scale_p' - scale_p'-1):
            what |G + d|^2 - |G|^2 can be for such a d
  resolved points, 1e-12 scale_p >= B_p: the issue's bound, unchanged;
  the others: |q_dev - q_host| <= B_p, an absolute bound, asserted on its own (at the wall-distance where it
            applies B_p ~ 1e-24 to 1e-12 against q ~ 1e+3 at the wall).
The numbers of points of either kind and both worst ratios are printed before they are asserted.
Under --np the output is unchanged (rank 0 writes the gathered solution with the host writer): byte-equal files."""
import os
import subprocess

import numpy as np
import pytest

from tests.test_gpu_app import G, tgv_prm
from tests.test_gpu_app_adaptive_dt import COUETTE
from tests.test_io import _read_vtu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12
NO_TIMER = "\nsubsection timer\n  set type = none\nend\n"


def run(tmp_path, name, prm, dim, *extra):
    d = tmp_path / name
    d.mkdir()
    (d / "case.prm").write_text(prm)
    app = os.path.join(ROOT, "apps", "gls_navier_stokes_%dd" % dim)
    if not os.path.exists(app):
        pytest.fail("%s is not built (run __graft_entry__.build())" % app)
    r = subprocess.run([app, *extra, "case.prm"], cwd=str(d), capture_output=True, text=True, timeout=170)
    assert r.returncode == 0, r.stderr[-3000:] + "\nstdout tail:\n" + r.stdout[-2000:]
    files = {f: (d / f).read_bytes() for f in sorted(os.listdir(d)) if f != "case.prm"}
    return r.stdout, files, d


def compare_pieces(fd, fh, dim, tag, smooth=False):
    """smooth: the q_criterion split of the module docstring (the cylinder); otherwise the issue's scale everywhere"""
    (npd, ncd, D), (nph, nch, H) = _read_vtu(fd), _read_vtu(fh)
    assert (npd, ncd) == (nph, nch) and list(D) == list(H)
    for n in ("connectivity", "offsets", "types", "subdomain"):
        assert D[n].tobytes() == H[n].tobytes(), (tag, n)
    om2 = (H["vorticity"].reshape(nph, -1) ** 2).sum(axis=1)
    npp = nph // nch if H["types"][0] in (70, 72) else None  # one Lagrange cell per patch
    assert npp, "the cases here write higher-order cells"
    scale = {"velocity": np.abs(H["velocity"]).max(), "pressure": np.abs(H["pressure"]).max(),
             "points": (H["points"].max(axis=0) - H["points"].min(axis=0)).max(),
             "vorticity": 0.5 * np.sqrt(om2.max()) if dim == 3 else 0.5 * np.abs(H["vorticity"]).max()}
    for n, s in scale.items():
        e = np.abs(D[n] - H[n]).max()
        print("%s %-12s max error %.3e scale %.3e" % (tag, n, e, s))
        assert e <= TOL * s, (tag, n, e, s)
    qs = np.abs(0.5 * np.cumsum(om2.reshape(-1, npp), axis=1).reshape(-1) - H["q_criterion"])
    e = np.abs(D["q_criterion"] - H["q_criterion"])
    ratio = e / np.maximum(TOL * qs, 1e-300)
    if not smooth:
        print("%s %-12s max error / (1e-12 scale) %.3e" % (tag, "q_criterion", ratio.max()))
        assert (e <= TOL * qs).all(), (tag, ratio.max())
        return
    X = H["points"].reshape(nch, npp, 3)
    dist = np.linalg.norm(X[:, :, None, :] - X[:, None, :, :], axis=3)
    hmin = np.where(dist > 0, dist, np.inf).min(axis=(1, 2))
    umax = np.linalg.norm(H["velocity"].reshape(nch, npp, 3), axis=2).max(axis=1)
    delta = 2.0 * 3 * 8 * dim * np.finfo(np.float64).eps * umax / hmin  # between two evaluations, per entry
    inc = np.diff(qs.reshape(nch, npp), axis=1, prepend=0.0).clip(min=0.0)
    B = np.cumsum(2.0 * np.sqrt(2.0 * inc) * dim * delta[:, None] + (dim * delta[:, None]) ** 2, axis=1).reshape(-1)
    resolved = TOL * qs >= B
    print("%s %-12s %d resolved points, max error / (1e-12 scale) %.3e; %d others, max error / absolute bound %.3e"
          % (tag, "q_criterion", resolved.sum(), ratio[resolved].max(initial=0.0), (~resolved).sum(),
             (e[~resolved] / np.maximum(B[~resolved], 1e-300)).max(initial=0.0)))
    assert resolved.any(), tag  # the wall cells: the issue's bound is not vacuous here
    assert (e[resolved] <= TOL * qs[resolved]).all(), (tag, ratio[resolved].max())
    assert (e[~resolved] <= B[~resolved]).all(), (tag, (e[~resolved] / np.maximum(B[~resolved], 1e-300)).max())


def cylinder_prm():
    t = open(os.path.join(ROOT, "apps", "cases", "cylinder3d_q2q1_re200.prm")).read()
    for a, b in [("set time end                = 0.25", "set time end = 0.1"),
                 ("set output frequency        = 1000000", "set output frequency = 1"),
                 ("set type                    = iteration", "set type = none"),
                 ("set file name               = cylinder3d_extruded.msh",
                  "set file name = " + os.path.join(ROOT, "apps", "cases", "cylinder3d_extruded.msh"))]:
        assert a in t, a
        t = t.replace(a, b)
    return t


def tgv_case():
    g = G["tgv_bdf1"]
    return tgv_prm("bdf1", 2, 1, 4, g["dt"], 2 * g["dt"], output_frequency=1) + NO_TIMER, 2, "tgv", 3


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["tgv_q2q1_2d", "cylinder3d_q2q1"])
def test_single_rank_device_output_equals_host_output(tmp_path, case):
    prm, dim, stem, n_out = tgv_case() if case.startswith("tgv") else (cylinder_prm(), 3, "cylinder3d", 3)
    out_d, files_d, dd = run(tmp_path, "device", prm, dim, "--output-eval", "device")
    out_h, files_h, dh = run(tmp_path, "host", prm, dim, "--output-eval", "host")
    assert out_d == out_h
    assert sorted(files_d) == sorted(files_h)
    pieces = [f for f in files_d if f.endswith(".vtu")]
    assert len(pieces) == n_out and stem + ".00002.00000.vtu" in pieces
    for f in files_d:
        if f.endswith(".vtu"):
            compare_pieces(str(dd / f), str(dh / f), dim, case + " " + f, smooth=case.startswith("cylinder"))
        else:
            assert files_d[f] == files_h[f], f


@pytest.mark.gpu
def test_two_ranks_output_is_unchanged(tmp_path):
    """--np 2 with the default options writes what --np 2 --output-eval host writes, byte for byte"""
    prm = COUETTE.replace("set output frequency             = 0", "set output frequency = 1\n  set output name = couette")
    assert "couette" in prm
    out_a, files_a, _ = run(tmp_path, "default", prm, 2, "--np", "2")
    out_b, files_b, _ = run(tmp_path, "host", prm, 2, "--np", "2", "--output-eval", "host")
    assert out_a == out_b
    assert sorted(files_a) == sorted(files_b) and any(f.endswith(".vtu") for f in files_a)
    for f in files_a:
        assert files_a[f] == files_b[f], f


@pytest.mark.gpu
def test_element_without_a_kernel_falls_back_to_the_host_writer(tmp_path):
    """2D Q3-Q3: gls_output_plan_create refuses the element, the default run writes with the host evaluation --
    the files of --output-eval host, byte for byte"""
    g = G["tgv_bdf1"]
    prm = tgv_prm("bdf1", 3, 3, 2, g["dt"], g["dt"], output_frequency=1) + NO_TIMER
    out_a, files_a, _ = run(tmp_path, "default", prm, 2)
    out_b, files_b, _ = run(tmp_path, "host", prm, 2, "--output-eval", "host")
    assert out_a == out_b
    assert sorted(files_a) == sorted(files_b) and "tgv.00001.00000.vtu" in files_a
    for f in files_a:
        assert files_a[f] == files_b[f], f
