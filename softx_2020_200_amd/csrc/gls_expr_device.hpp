// gls_expr_device.hpp -- the device interpreter of a gls_expr's stack bytecode (gls_expr_program.hpp), included by
// the kernels that evaluate an expression: gls_expr_device.hip (gls_expr_eval_device) and gls_error.hip (the exact
// solution at the Gauss points). The semantics are run_code's in gls_io.cpp, operation by operation.
//
// All lanes of a launch run the same program: the instruction is read through a wave-uniform index and its opcode
// and index are made scalar (readfirstlane), so both switches are uniform branches. The operand stack is in LDS as
// stack[depth][block]: lane t's entry d is st[d * block] with st = stack + t, a wave reads and writes 64
// consecutive doubles, and nothing is indexed per lane by a run-time value in registers (which would go to
// scratch). Every value passes through the stack between two operations and contraction is off in the
// interpreter, so a MUL followed by an ADD stays two rounded operations as on the host.
#pragma once
#include <hip/hip_runtime.h>

#include "gls_expr_program.hpp"

namespace gls {
namespace expr {

// the program on the device: component c is code[off[c] .. off[c + 1])
struct DeviceProgram {
  const FlatInstr *code = nullptr;
  const int32_t *off = nullptr;
  int n_vars = 0, n_comps = 0, max_stack = 0;
};

// gls_expr_device.hip: the device copy of an expression's program, uploaded at the first call and owned by the
// expression. GLS_EINVAL (with a message) for a program whose stack is deeper than kDeviceMaxStack.
int device_program(const gls_expr *e, const char *who, DeviceProgram *out);

#ifdef __HIP__
// The functions are called, not inlined: inlined into the interpreter's loop the constants of 30 math routines are
// hoisted out of it and fill the register file (256 VGPRs and AGPR copies; 120 VGPRs this way). No scratch either way.
inline __device__ __noinline__ double apply_fun1(int f, double x) {
  switch (f) {
    case F_SIN: return sin(x);
    case F_COS: return cos(x);
    case F_TAN: return tan(x);
    case F_ASIN: return asin(x);
    case F_ACOS: return acos(x);
    case F_ATAN: return atan(x);
    case F_SINH: return sinh(x);
    case F_COSH: return cosh(x);
    case F_TANH: return tanh(x);
    case F_ASINH: return asinh(x);
    case F_ACOSH: return acosh(x);
    case F_ATANH: return atanh(x);
    case F_LOG2: return log2(x);
    case F_LOG10: return log10(x);
    case F_LOG:
    case F_LN: return log(x);
    case F_EXP: return exp(x);
    case F_SQRT: return sqrt(x);
    case F_SIGN: return (double)((x > 0) - (x < 0));
    case F_RINT: return rint(x);
    case F_ABS: return fabs(x);
    case F_INT: return (double)llround(x);  // deal.II mu_round
    case F_CEIL: return ceil(x);
    case F_FLOOR: return floor(x);
    case F_COT: return 1.0 / tan(x);
    case F_CSC: return 1.0 / sin(x);
    case F_SEC: return 1.0 / cos(x);
    case F_ERFC: return erfc(x);
    case F_ERF: return erf(x);
    default: return x;
  }
}

inline __device__ __noinline__ double apply_fun2(int f, double a, double b) {
  switch (f) {
    case F_ATAN2: return atan2(a, b);
    case F_POW: return pow(a, b);
    default: return fmod(a, b);
  }
}

// one component on the calling lane. st: the lane's column of the LDS stack (entry d at st[d * BLOCK], BLOCK the
// lanes of the block), var(i): the lane's value of variable i (i is wave-uniform). No barrier inside: lanes
// without a point may skip the call.
template <class Var>
__device__ __forceinline__ double run(const FlatInstr *__restrict__ code, int begin, int end, double *st,
                                      const int BLOCK, Var var) {
#pragma clang fp contract(off)
  int sp = 0;
  for (int pc = begin; pc < end; ++pc) {
    const int op = __builtin_amdgcn_readfirstlane(code[pc].op), ii = __builtin_amdgcn_readfirstlane(code[pc].i);
    switch (op) {
      case PUSH_C: st[sp++ * BLOCK] = code[pc].c; break;
      case PUSH_V: st[sp++ * BLOCK] = var(ii); break;
      case NEG: st[(sp - 1) * BLOCK] = -st[(sp - 1) * BLOCK]; break;
      case NOT: st[(sp - 1) * BLOCK] = st[(sp - 1) * BLOCK] == 0.0 ? 1.0 : 0.0; break;
      case F1: st[(sp - 1) * BLOCK] = apply_fun1(ii, st[(sp - 1) * BLOCK]); break;
      case F2: {
        --sp;
        const double a = st[(sp - 1) * BLOCK], b = st[sp * BLOCK];
        st[(sp - 1) * BLOCK] = apply_fun2(ii, a, b);
        break;
      }
      case SEL: {  // both branches are on the stack already
        sp -= 2;
        const double c = st[(sp - 1) * BLOCK], a = st[sp * BLOCK], b = st[(sp + 1) * BLOCK];
        st[(sp - 1) * BLOCK] = c != 0.0 ? a : b;
        break;
      }
      case FMIN:
      case FMAX:
      case FSUM: {
        double r = st[(sp - ii) * BLOCK];
        for (int k = 1; k < ii; ++k) {
          const double v = st[(sp - ii + k) * BLOCK];
          r = op == FMIN ? (v < r ? v : r) : op == FMAX ? (r < v ? v : r) : r + v;  // std::min / std::max (r, v)
        }
        sp -= ii - 1;
        st[(sp - 1) * BLOCK] = r;
        break;
      }
      default: {
        --sp;
        const double a = st[(sp - 1) * BLOCK], b = st[sp * BLOCK];
        double r = 0.;
        switch (op) {
          case ADD: r = a + b; break;
          case SUB: r = a - b; break;
          case MUL: r = a * b; break;
          case DIV: r = a / b; break;
          case POW: r = apply_fun2(F_POW, a, b); break;
          case LT: r = a < b; break;
          case GT: r = a > b; break;
          case LE: r = a <= b; break;
          case GE: r = a >= b; break;
          case EQ: r = a == b; break;
          case NE: r = a != b; break;
          case AND: r = (a != 0.0) && (b != 0.0); break;
          case OR: r = (a != 0.0) || (b != 0.0); break;
        }
        st[(sp - 1) * BLOCK] = r;
      }
    }
  }
  return st[0];
}
#endif  // __HIP__

}  // namespace expr
}  // namespace gls
