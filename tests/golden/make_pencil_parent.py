"""Generate tests/golden/pencil_parent.json (and pencil_parent.npz where needed): what the pencil kernels computed at
the commit before their index bookkeeping was rewritten, for tests/test_gpu_pencil_bookkeeping.py.

Run once on the GPU with that commit's library (the cases and how they run are test_gpu_pencil_bookkeeping.py's
SHAPES / SCHEMES / GATHERS / run_case). Every (n, scheme) runs twice, each time on a freshly built hierarchy. A
quantity whose two runs agree bit for bit is stored as the SHA-256 of its bytes; one whose runs differ (only the
rocSOLVER / rocBLAS routes of apply_preconditioner can) as the first run's vector in pencil_parent.npz with the
tolerance 10 x max|a1 - a2| / max|a1| (floor 1e-14) next to it.

    python tests/golden/make_pencil_parent.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from tests.test_gpu_pencil_bookkeeping import GATHERS, SCHEMES, SHAPES, case_name, digest, run_case  # noqa: E402


def main():
    cases, vectors = {}, {}
    for n in SHAPES:
        for scheme in SCHEMES:
            r1, r2 = run_case(n, scheme), run_case(n, scheme)
            for gather in GATHERS:
                name, entry = case_name(n, scheme, gather), {}
                for q, a1 in r1[gather].items():
                    a2 = r2[gather][q]
                    if q == "fused":
                        assert a1 == a2, (name, a1, a2)
                        entry[q] = list(a1)
                        continue
                    assert np.isfinite(a1).all() and np.abs(a1).max() > 0, (name, q)
                    e = {"size": int(a1.size)}
                    if np.array_equal(a1, a2):
                        e["sha256"] = digest(a1)
                    else:
                        e["parent_vs_parent"] = float(np.abs(a1 - a2).max() / np.abs(a1).max())
                        e["tolerance"] = max(10.0 * e["parent_vs_parent"], 1e-14)
                        vectors[name + ":" + q] = a1
                    entry[q] = e
                cases[name] = entry
                print(name, {q: (e if q == "fused" else e.get("sha256", "")[:12] or e) for q, e in entry.items()},
                      flush=True)
    with open(os.path.join(HERE, "pencil_parent.json"), "w") as f:
        json.dump({"cases": cases}, f, indent=1, sort_keys=True)
        f.write("\n")
    if vectors:
        np.savez_compressed(os.path.join(HERE, "pencil_parent.npz"), **vectors)
    print("wrote %d cases, %d quantities as vectors" % (len(cases), len(vectors)))


if __name__ == "__main__":
    main()
