"""CPU-side checks of the projection entry points (no GPU calls): include/gls_native.h declares them, the library
exports them, the binding lists them, and a null context is refused with a message instead of a crash."""
import ctypes as C
import os
import re

from softx_2020_200_amd.native import EXPORTS, GLS_EINVAL, ProjectionInfo, load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["gls_projection_plan_create", "gls_projection_plan_destroy", "gls_mass_apply", "gls_mass_diagonal",
           "gls_l2_projection"]


def test_projection_symbols_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "gls_native.h")).read()
    declared = set(re.findall(r"^(?:int|void|const char \*)\s*(gls_\w+)\s*\(", hdr, re.M))
    L = load()
    for name in SYMBOLS:
        assert name in declared and name in EXPORTS and hasattr(L, name), name
    assert "typedef struct { int iterations; double relative_residual; } gls_projection_info;" in hdr
    assert [f[0] for f in ProjectionInfo._fields_] == ["iterations", "relative_residual"]


def test_null_context_is_refused():
    L = load()
    plan, info = C.c_void_p(), ProjectionInfo()
    assert L.gls_projection_plan_create(None, None, C.byref(plan)) == GLS_EINVAL
    assert b"null context" in L.gls_last_error()
    assert L.gls_mass_apply(None, None, None, None) == GLS_EINVAL
    assert L.gls_mass_diagonal(None, None, None) == GLS_EINVAL
    assert L.gls_l2_projection(None, None, None, 0.0, None, C.byref(info)) == GLS_EINVAL
    assert L.gls_projection_plan_destroy(None) == 0
