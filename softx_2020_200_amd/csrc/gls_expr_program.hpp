// gls_expr_program.hpp -- the stack bytecode of a gls_expr as plain data: what the parser in gls_io.cpp emits, what
// run_code there interprets on the host and what gls_expr_device.hpp interprets on the device. The opcodes and the
// function indices are shared so that the two interpreters cannot number them differently.
#pragma once
#include <cstdint>
#include <vector>

struct gls_expr;

namespace gls {
namespace expr {

enum Op : int {
  PUSH_C, PUSH_V, NEG, ADD, SUB, MUL, DIV, POW, LT, GT, LE, GE, EQ, NE, AND, OR, NOT, SEL, F1, F2, FMIN, FMAX, FSUM
};

// index of a one-argument function: the order of kFun1 in gls_io.cpp
enum Fun1Index : int {
  F_SIN, F_COS, F_TAN, F_ASIN, F_ACOS, F_ATAN, F_SINH, F_COSH, F_TANH, F_ASINH, F_ACOSH, F_ATANH, F_LOG2, F_LOG10,
  F_LOG, F_LN, F_EXP, F_SQRT, F_SIGN, F_RINT, F_ABS, F_INT, F_CEIL, F_FLOOR, F_COT, F_CSC, F_SEC, F_ERFC, F_ERF,
  F1_COUNT
};
// index of a two-argument function: the order of kFun2 in gls_io.cpp
enum Fun2Index : int { F_ATAN2, F_POW, F_FMOD, F2_COUNT };

// one instruction: i = variable index (PUSH_V), function index (F1, F2) or argument count (FMIN, FMAX, FSUM)
struct FlatInstr {
  int32_t op, i;
  double c;
};

// the components of one expression back to back: component c is code[off[c] .. off[c + 1])
struct FlatProgram {
  std::vector<FlatInstr> code;
  std::vector<int32_t> off;
  int n_vars = 0, n_comps = 0, max_stack = 0;
};

constexpr int kDeviceMaxStack = 16;  // operand stack entries per lane of the device interpreter

}  // namespace expr
}  // namespace gls

// gls_io.cpp: the program of an expression, and the slot where gls_expr keeps its device copy (owned by the
// expression: gls_expr_destroy hands it to gls::expr::device_release)
void gls_io_expr_flatten(const gls_expr *e, gls::expr::FlatProgram &out);
void **gls_io_expr_device_slot(const gls_expr *e);

namespace gls {
namespace expr {
// gls_expr_device.hip
void device_release(void *device_copy);
}  // namespace expr
}  // namespace gls
