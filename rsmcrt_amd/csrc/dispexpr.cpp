// dispexpr.cpp — smcrt_displacement_compile / _eval / _describe (smcrt.h "displacement
// expressions"): a recursive-descent parser that emits the postfix program as it goes, with no
// rewriting, so the operations and their order are the ones written.
#include "dispexpr.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "hosterr.h"

namespace smcrt {
namespace {

constexpr int DX_MAX_PARENS = 64;  // nested parentheses and unary minuses (the parser's recursion)

struct Fn {
  const char* name;
  uint32_t op;
  int args;
};
const Fn FNS[] = {{"abs", DX_ABS, 1},     {"sqrt", DX_SQRT, 1}, {"sin", DX_SIN, 1}, {"cos", DX_COS, 1},
                  {"floor", DX_FLOOR, 1}, {"min", DX_MIN, 2},   {"max", DX_MAX, 2}};

struct Compiler {
  const char* s;
  size_t i = 0;
  std::vector<unsigned char> code;
  std::vector<double> consts;
  int depth = 0, nest = 0;
  std::string err;  // the first error

  bool fail(size_t at, const std::string& m) {
    if (err.empty()) err = "displacement expression, column " + std::to_string(at + 1) + ": " + m;
    return false;
  }
  void skip() {
    while (s[i] == ' ' || s[i] == '\t' || s[i] == '\n' || s[i] == '\r') ++i;
  }
  bool emit(uint32_t op, size_t at) {
    if ((int)code.size() >= DX_MAX_CODE) return fail(at, "more than " + std::to_string(DX_MAX_CODE) + " instructions");
    depth += 1 - dx_arity(op);
    if (depth > DX_MAX_STACK)
      return fail(at, "needs more than " + std::to_string(DX_MAX_STACK) + " stack values (parenthesise from the left)");
    code.push_back((unsigned char)op);
    return true;
  }
  bool constant(double v, size_t at) {
    if (!std::isfinite(v)) return fail(at, "constant is not finite");
    size_t k = 0;
    while (k < consts.size() && std::memcmp(&consts[k], &v, sizeof v) != 0) ++k;
    if (k == consts.size()) {
      if ((int)k >= DX_MAX_CONSTS) return fail(at, "more than " + std::to_string(DX_MAX_CONSTS) + " distinct constants");
      consts.push_back(v);
    }
    return emit(DX_CONST + (uint32_t)k, at);
  }
  static bool digit(char c) { return c >= '0' && c <= '9'; }
  static bool alpha(char c) { return (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z') || c == '_'; }
  bool at_number() { return digit(s[i]) || (s[i] == '.' && digit(s[i + 1])); }
  bool number(bool negate) {
    const size_t at = i;
    char* end = nullptr;
    const double v = std::strtod(s + i, &end);
    if (end == s + i) return fail(at, "bad number");
    i = (size_t)(end - s);
    return constant(negate ? -v : v, at);
  }
  bool expect(char c) {
    skip();
    if (s[i] != c) return fail(i, std::string("expected '") + c + "'");
    ++i;
    return true;
  }

  bool primary() {
    skip();
    const size_t at = i;
    if (at_number()) return number(false);
    if (s[i] == '(') {
      ++i;
      if (++nest > DX_MAX_PARENS) return fail(at, "nested too deeply");
      if (!expr()) return false;
      --nest;
      return expect(')');
    }
    if (alpha(s[i])) {
      size_t e = i;
      while (alpha(s[e]) || digit(s[e])) ++e;
      const std::string name(s + i, e - i);
      i = e;
      if (name == "x") return emit(DX_X, at);
      if (name == "y") return emit(DX_Y, at);
      if (name == "z") return emit(DX_Z, at);
      if (name == "pi") return constant(3.14159265358979323846, at);
      for (const Fn& f : FNS) {
        if (name != f.name) continue;
        if (!expect('(')) return false;
        if (++nest > DX_MAX_PARENS) return fail(at, "nested too deeply");
        if (!expr()) return false;
        if (f.args == 2 && !(expect(',') && expr())) return false;
        --nest;
        skip();
        if (s[i] == ',') return fail(i, name + " takes " + std::to_string(f.args) + (f.args == 1 ? " argument" : " arguments"));
        return expect(')') && emit(f.op, at);
      }
      return fail(at, "unknown name '" + name + "'");
    }
    return fail(at, s[i] ? std::string("unexpected '") + s[i] + "'" : std::string("unexpected end of the expression"));
  }
  bool unary() {
    skip();
    if (s[i] != '-') return primary();
    const size_t at = i++;
    skip();
    if (at_number()) return number(true);  // the literal negated: the same value as negating it
    if (++nest > DX_MAX_PARENS) return fail(at, "nested too deeply");
    if (!unary()) return false;
    --nest;
    return emit(DX_NEG, at);
  }
  bool term() {
    if (!unary()) return false;
    for (;;) {
      skip();
      const char c = s[i];
      if (c != '*' && c != '/') return true;
      const size_t at = i++;
      if (!unary() || !emit(c == '*' ? DX_MUL : DX_DIV, at)) return false;
    }
  }
  bool expr() {
    if (!term()) return false;
    for (;;) {
      skip();
      const char c = s[i];
      if (c != '+' && c != '-') return true;
      const size_t at = i++;
      if (!term() || !emit(c == '+' ? DX_ADD : DX_SUB, at)) return false;
    }
  }
  bool all() {
    if (!expr()) return false;
    skip();
    if (s[i]) return fail(i, std::string("unexpected '") + s[i] + "'");
    return true;
  }
};

const smcrt_sdf_node* program_node(const smcrt_sdf_node* node, const char* who) {
  std::string why;
  if (!node || node->kind != SMCRT_SDF_DISPLACEMENT || node->param[0] != (double)SMCRT_DISP_EXPR) {
    set_error(SMCRT_ERR_INVALID_ARG, std::string(who) + ": not a displacement node with an expression");
    return nullptr;
  }
  if (!disp_expr_verify(*node, &why)) {
    set_error(SMCRT_ERR_INVALID_ARG, std::string(who) + ": bad expression program: " + why);
    return nullptr;
  }
  return node;
}

}  // namespace
}  // namespace smcrt

using namespace smcrt;

extern "C" int smcrt_displacement_compile(const char* expr, smcrt_sdf_node* node) {
  if (!expr || !node) return set_error(SMCRT_ERR_INVALID_ARG, "smcrt_displacement_compile: null argument");
  Compiler c{expr};
  if (!c.all()) return set_error(SMCRT_ERR_INVALID_ARG, c.err);
  node->kind = SMCRT_SDF_DISPLACEMENT;
  for (double& t : node->transform) t = 0.0;
  for (double& p : node->param) p = 0.0;
  node->param[0] = (double)SMCRT_DISP_EXPR;
  node->param[DX_LEN_PARAM] = (double)c.code.size();
  node->param[DX_NCONST_PARAM] = (double)c.consts.size();
  std::memcpy(node->param + DX_CODE_PARAM, c.code.data(), c.code.size());
  for (size_t k = 0; k < c.consts.size(); ++k) node->transform[k] = c.consts[k];
  return SMCRT_OK;
}

extern "C" int smcrt_displacement_eval(const smcrt_sdf_node* node, const double* xyz, int64_t n, double* out) {
  if (n < 0 || (n > 0 && (!xyz || !out))) return set_error(SMCRT_ERR_INVALID_ARG, "smcrt_displacement_eval: bad arguments");
  if (!program_node(node, "smcrt_displacement_eval")) return SMCRT_ERR_INVALID_ARG;
  for (int64_t i = 0; i < n; ++i) out[i] = disp_expr_value(node, 0, v3(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]));
  return SMCRT_OK;
}

extern "C" int smcrt_displacement_describe(const smcrt_sdf_node* node, char* buf, int32_t cap) {
  if (!buf || cap < 1) return set_error(SMCRT_ERR_INVALID_ARG, "smcrt_displacement_describe: bad arguments");
  if (!program_node(node, "smcrt_displacement_describe")) return SMCRT_ERR_INVALID_ARG;
  static const char* const BIN[] = {" + ", " - ", " * ", " / "};
  unsigned char code[DX_MAX_CODE];
  dx_code(*node, code);
  std::vector<std::string> st;
  for (int i = 0; i < (int)node->param[DX_LEN_PARAM]; ++i) {
    const uint32_t op = code[i];
    if (dx_arity(op) == 0) {
      if (op >= DX_CONST) {
        char num[40];
        std::snprintf(num, sizeof num, "%.17g", node->transform[op - DX_CONST]);
        st.push_back(num);
      } else {
        st.push_back(op == DX_X ? "x" : op == DX_Y ? "y" : "z");
      }
    } else if (dx_arity(op) == 2) {
      const std::string b = st.back();
      st.pop_back();
      std::string& a = st.back();
      if (op == DX_MIN || op == DX_MAX) a = std::string(op == DX_MIN ? "min(" : "max(") + a + ", " + b + ")";
      else a = "(" + a + BIN[op - DX_ADD] + b + ")";
    } else if (op == DX_NEG) {
      st.back() = "(-(" + st.back() + "))";  // (not "-" before a number, which would be a constant)
    } else {
      for (const Fn& f : FNS)
        if (f.op == op) st.back() = std::string(f.name) + "(" + st.back() + ")";
    }
  }
  const std::string& text = st.back();
  if ((size_t)cap < text.size() + 1)
    return set_error(SMCRT_ERR_INVALID_ARG, "smcrt_displacement_describe: needs " + std::to_string(text.size() + 1) + " bytes");
  std::memcpy(buf, text.c_str(), text.size() + 1);
  return SMCRT_OK;
}
