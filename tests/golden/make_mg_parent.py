"""Generate tests/golden/mg_parent.json (and mg_parent.npz where needed): the multigrid's results at the commit
before it moved out of gls_api.cpp, for tests/test_gpu_mg_split.py.

Run once on the GPU at that commit (the cases and how they run are test_gpu_mg_split.py's CASES / run_case). Every
case runs twice, each time on a freshly built hierarchy. A case whose two runs agree bit for bit is stored as the
SHA-256 of apply_preconditioner(v)'s bytes; one whose runs differ (only the rocSOLVER / rocBLAS routes can) as the
first run's vector in mg_parent.npz with the tolerance 10 x max|z1 - z2| / max|z1| (floor 1e-14) next to it. The GMRES
iteration count of solve_linear(residual, relative_residual=1e-8) is stored for every case and must repeat.

    python tests/golden/make_mg_parent.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from tests.test_gpu_mg_split import CASES, digest, run_case  # noqa: E402


def main():
    cases, vectors = {}, {}
    for name in CASES:
        (z1, its1), (z2, its2) = run_case(name), run_case(name)
        assert its1 == its2, (name, its1, its2)
        e = {"n_dofs": int(z1.size), "gmres_its": its1}
        if np.array_equal(z1, z2):
            e["sha256"] = digest(z1)
        else:
            e["parent_vs_parent"] = float(np.abs(z1 - z2).max() / np.abs(z1).max())
            e["tolerance"] = max(10.0 * e["parent_vs_parent"], 1e-14)
            vectors[name] = z1
        cases[name] = e
        print(name, e, flush=True)
    with open(os.path.join(HERE, "mg_parent.json"), "w") as f:
        json.dump({"cases": cases}, f, indent=1, sort_keys=True)
        f.write("\n")
    if vectors:
        np.savez_compressed(os.path.join(HERE, "mg_parent.npz"), **vectors)
    print("wrote %d cases, %d as vectors" % (len(cases), len(vectors)))


if __name__ == "__main__":
    main()
