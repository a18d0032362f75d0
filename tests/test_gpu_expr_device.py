"""The device interpreter of the expression bytecode (gls_expr_eval_device through Expr.eval_device) against the
host evaluator (gls_expr_eval, Expr.__call__) on the same values: one expression per opcode and per function name
of the kFun1 / kFun2 tables of csrc/gls_io.cpp (the names are read from the source, so a wrong table index shows as
a gross error).

257 points (four waves and one lane: the last block is partial), seeded x in U(0.1, 0.9), y in U(1.1, 3),
z in U(-2, 2), t = 0.3; every function gets an argument inside its domain.

Two classes. Bitwise: + - * and unary minus, the comparisons, && || ! and ?:, abs floor ceil rint int sign,
min max sum, constants and variables -- the device executes the host's operation. Capped: / sqrt ^ pow and the
transcendental functions are within 32 ulp of the host's value: the loosest published double-precision bound
for such functions (16 ulp) with room for glibc's own error; a wrong dispatch misses it by many orders of
magnitude. The measured maximum per function is printed."""
import os
import re

import numpy as np
import pytest

from softx_2020_200_amd.io import Expr
from softx_2020_200_amd.native import GLSError
from tests.gpu_util import cuda

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20200200
N = 257
ULP_CAP = 32.0
STACK_CAP = 16
VARS = "x,y,z,t"


def table_names(table):
    src = open(os.path.join(ROOT, "softx_2020_200_amd", "csrc", "gls_io.cpp")).read()
    body = re.search(r"const Fun\d %s\[\] = \{(.*?)\};" % table, src, re.S).group(1)
    return re.findall(r'\{"(\w+)",', body)


FUN1, FUN2 = table_names("kFun1"), table_names("kFun2")

# the argument of each one-argument function (inside its domain); default: z
ARG1 = dict(asin="x", acos="x", atanh="x", acosh="y", log2="y", log10="y", log="y", ln="y", sqrt="y", tan="x", cot="x",
            csc="x", sec="x", sign="z", rint="3*z", abs="z", int="3*z", ceil="3*z", floor="3*z")
ARG2 = dict(atan2="z, x", pow="y, z", fmod="3*z, y")
BITWISE_FUN1 = {"abs", "floor", "ceil", "rint", "int", "sign"}

BITWISE = {
    "add": "x + y", "sub": "x - z", "mul": "y * z", "neg": "-z", "mul_then_add": "x * y + z * t",
    "lt": "z < x", "gt": "z > x", "le": "z <= 0.5", "ge": "y >= 2", "eq": "rint(z) == 1", "ne": "rint(z) != 0",
    "and": "(z > 0) && (x > 0.5)", "or": "(z > 1) || (x < 0.3)", "not": "!(z > 0)", "not_value": "!rint(x)",
    "ternary": "z > 0 ? x : y", "if": "if(z < x, y, -y)",
    "min": "min(x, y, z, t)", "max": "max(z, x, t)", "sum": "sum(x, y, z, t, 1.5)", "min1": "min(z)",
    "constant": "2.5", "pi": "pi", "variable_t": "t", "variable_z": "z",
}
BITWISE.update({"fun_" + f: "%s(%s)" % (f, ARG1.get(f, "z")) for f in FUN1 if f in BITWISE_FUN1})
CAPPED = {"div": "x / y", "pow_op": "x ^ y", "pow_op_neg": "y ^ (-z)", "avg": "avg(x, y, z)"}
CAPPED.update({"fun_" + f: "%s(%s)" % (f, ARG1.get(f, "z")) for f in FUN1 if f not in BITWISE_FUN1})
CAPPED.update({"fun_" + f: "%s(%s)" % (f, ARG2[f]) for f in FUN2})


def values(n=N):
    rng = np.random.default_rng(SEED)
    return np.stack([rng.uniform(0.1, 0.9, n), rng.uniform(1.1, 3.0, n), rng.uniform(-2.0, 2.0, n), np.full(n, 0.3)], axis=1)


def both(expression, v, variables=VARS, constants=""):
    e = Expr(expression, variables, constants)
    return e(v), e.eval_device(cuda(v)).cpu().numpy()


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def ulps(dev, host):
    return np.abs(dev - host) / np.spacing(np.abs(host))


def test_the_tables_are_read():
    assert len(FUN1) == 29 and len(FUN2) == 3, (FUN1, FUN2)
    assert set(ARG1) <= set(FUN1) and set(ARG2) == set(FUN2)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(BITWISE))
def test_bitwise_class(name):
    host, dev = both(BITWISE[name], values())
    assert np.isfinite(host).all()
    assert same_bits(host, dev), (name, BITWISE[name], np.abs(host - dev).max())


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CAPPED))
def test_capped_class(name):
    host, dev = both(CAPPED[name], values())
    assert np.isfinite(host).all() and np.isfinite(dev).all(), name
    u = ulps(dev, host).max()
    print("max ulp %-12s %-16s %.2f" % (name, CAPPED[name], u))
    assert u <= ULP_CAP, (name, CAPPED[name], u)


@pytest.mark.gpu
def test_three_components_with_constants():
    v = values()
    host, dev = both("a*x + b; sin(a*y) * z; b - t*z", v, constants="a=1.75, b=-0.5")
    assert host.shape == dev.shape == (N, 3)
    assert same_bits(host[:, 0], dev[:, 0]) and same_bits(host[:, 2], dev[:, 2])
    assert ulps(dev[:, 1], host[:, 1]).max() <= ULP_CAP


@pytest.mark.gpu
def test_nested_ternary_with_nan_in_the_untaken_branch():
    """both branches are evaluated (SEL): the NaN of the untaken one must not leak, and where the host gives NaN
    the device gives NaN"""
    v = values()
    v[:, 0] = np.where(np.arange(N) % 2 == 0, v[:, 0], -v[:, 0])  # both signs of x
    host, dev = both("x > 0 ? (y > 2 ? sqrt(x) : -sqrt(x)) : sqrt(-x)", v)
    assert np.isfinite(host).all() and same_bits(host, dev)  # sqrt is correctly rounded on both sides
    host, dev = both("x > 0 ? sqrt(-x) : 1", v)
    assert np.isnan(host[::2]).all() and np.array_equal(np.isnan(host), np.isnan(dev))
    assert same_bits(host[1::2], dev[1::2])


def right_nested_sum(depth):
    """x + (x + (... + x)): `depth` operands are on the stack before the first ADD"""
    return "x + (" * (depth - 1) + "x" + ")" * (depth - 1)


@pytest.mark.gpu
def test_stack_depth_at_the_cap_and_past_it():
    v = values()
    host, dev = both(right_nested_sum(STACK_CAP), v)
    assert same_bits(host, dev)
    e = Expr(right_nested_sum(STACK_CAP + 1), VARS)
    assert np.isfinite(e(v)).all()  # the host evaluates it
    with pytest.raises(GLSError, match="stack of %d" % (STACK_CAP + 1)):
        e.eval_device(cuda(v))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1])
def test_point_counts(n):
    v = values(max(n, 1))[:n]
    host, dev = both("x * y - z; t", v)
    assert host.shape == dev.shape == (n, 2) and same_bits(host, dev)


@pytest.mark.gpu
def test_two_calls_are_bitwise_equal():
    e = Expr("exp(-t) * sin(pi*x) * cos(pi*y) + z^3; atan2(z, x)", VARS)
    v = cuda(values(3 * N))
    assert same_bits(e.eval_device(v).cpu().numpy(), e.eval_device(v).cpu().numpy())
