// dispexpr.h — the host side of SMCRT_DISP_EXPR: the check every stored displacement program
// passes before a scene takes its node (inline: sceneplan.cpp's validate() calls it, and the
// scene-plan probe links nothing else). The compiler and describe are in dispexpr.cpp; the
// interpreter, with the opcodes and limits, is geometry.h disp_expr_run.
#pragma once
#include <cstring>
#include <string>

#include "geometry.h"

namespace smcrt {

// The number of stack values an opcode pops (push: 0, unary: 1, binary: 2), -1 if unknown.
inline int dx_arity(uint32_t op) {
  if ((op >= DX_X && op <= DX_Z) || (op >= DX_CONST && op < DX_CONST + DX_MAX_CONSTS)) return 0;
  if (op >= DX_ADD && op <= DX_MAX) return 2;
  if (op >= DX_NEG && op <= DX_FLOOR) return 1;
  return -1;
}

inline void dx_code(const smcrt_sdf_node& nd, unsigned char code[DX_MAX_CODE]) {
  std::memcpy(code, nd.param + DX_CODE_PARAM, DX_MAX_CODE);
}

// A displacement node with param[0] == SMCRT_DISP_EXPR holds a program the interpreter may run:
// lengths within the node, known opcodes, constant indices below the constant count, zero
// padding after the last instruction (the interpreter stops there), and a stack that never
// underflows, never exceeds DX_MAX_STACK and ends with exactly one value.
inline bool disp_expr_verify(const smcrt_sdf_node& nd, std::string* why) {
  auto bad = [&](const std::string& m) {
    if (why) *why = m;
    return false;
  };
  const double len = nd.param[DX_LEN_PARAM], nc = nd.param[DX_NCONST_PARAM];
  if (!(len >= 1.0 && len <= (double)DX_MAX_CODE) || len != (double)(int)len)
    return bad("program length is not an integer in 1.." + std::to_string(DX_MAX_CODE));
  if (!(nc >= 0.0 && nc <= (double)DX_MAX_CONSTS) || nc != (double)(int)nc)
    return bad("constant count is not an integer in 0.." + std::to_string(DX_MAX_CONSTS));
  const int n = (int)len, n_const = (int)nc;
  unsigned char code[DX_MAX_CODE];
  dx_code(nd, code);
  int depth = 0;
  for (int i = 0; i < n; ++i) {
    const uint32_t op = code[i];
    const int ar = dx_arity(op);
    if (ar < 0) return bad("instruction " + std::to_string(i) + ": unknown opcode " + std::to_string(op));
    if (op >= DX_CONST && (int)(op - DX_CONST) >= n_const)
      return bad("instruction " + std::to_string(i) + ": constant index out of range");
    if (depth < ar) return bad("instruction " + std::to_string(i) + ": stack underflow");
    depth += 1 - ar;
    if (depth > DX_MAX_STACK) return bad("instruction " + std::to_string(i) + ": stack deeper than " + std::to_string(DX_MAX_STACK));
  }
  if (depth != 1) return bad("program leaves " + std::to_string(depth) + " values");
  for (int i = n; i < DX_MAX_CODE; ++i)
    if (code[i] != DX_END) return bad("code after the last instruction");
  return true;
}

}  // namespace smcrt
