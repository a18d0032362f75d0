"""The `forces` prm section of the application (parameters.cc:227-294) is validated while the file is read,
before the GPU is touched: an unknown verbosity dies as in the other sections, and the two frequencies are
step moduli (>= 1)."""
import pytest

from tests.test_io import _app


@pytest.mark.parametrize("text,msg", [
    ("subsection forces\n set verbosity = loud\nend\n", "Unknown verbosity mode for the forces"),
    ("subsection forces\n set calculate forces = maybe\nend\n", "is not a bool"),
    ("subsection forces\n set calculate forces = true\n set calculation frequency = 0\nend\n", "must be >= 1"),
    ("subsection forces\n set calculate torques = true\n set output frequency = 0\nend\n", "must be >= 1"),
])
def test_app_rejects_bad_forces_entries(tmp_path, text, msg):
    out = _app(tmp_path, text, "--dim", "2")
    assert out.returncode == 1 and msg in out.stderr, out.stderr
