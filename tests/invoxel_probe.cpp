// invoxel_probe — a stand-alone host program (g++ -O2 -ffp-contract=off, no HIP) that checks
// rsmcrt_amd/csrc/invoxel.h against a literal restatement of the first crossing of update_grids
// (inttau2.f90:417-429 with wall_dist :467-521: exact divisions, the -999 / 100000 rules,
// d + dcell > len with d = 0).
//
//   invoxel_probe SEED N_RANDOM N_COMPLETE
//
// Soundness: over N_RANDOM seeded random cases and the adversarial families below, a case
// where the predicate is true but the restatement does not end in its start voxel without an
// error stop is a violation. Completeness: over N_COMPLETE cases drawn like M1's segments the
// share of true one-crossing segments the predicate accepts, and the share far.h's form
// (refined reciprocal, 2^-40 margin) accepts on the same cases. Prints key=value lines.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../rsmcrt_amd/csrc/invoxel.h"

namespace {

struct Rng {  // splitmix64
  uint64_t s;
  uint64_t next() {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  double uni() { return (double)(next() >> 11) * 0x1.0p-53; }                // [0, 1)
  double range(double a, double b) { return a + (b - a) * uni(); }
  int below(int n) { return (int)(next() % (uint64_t)n); }
};

double ulps(double x, int m) {  // x moved by m representable numbers
  const double to = m > 0 ? INFINITY : -INFINITY;
  for (int i = 0; i < std::abs(m); ++i) x = std::nextafter(x, to);
  return x;
}

// ---- the reference's first crossing: true iff it is the last one and no error stop ----------
bool ref_single(const double f[3], const double o[3], const double dir[3], double len, double* dcell_out) {
  double d[3];
  for (int a = 0; a < 3; ++a) {
    d[a] = -999.0;
    if (dir[a] > 0.0 || dir[a] < 0.0) d[a] = (f[a] - o[a]) / dir[a];
    else if (dir[a] == 0.0) d[a] = 100000.0;
  }
  double dcell = d[0] < d[1] ? d[0] : d[1];
  dcell = dcell < d[2] ? dcell : d[2];
  if (std::isnan(d[0]) || std::isnan(d[1]) || std::isnan(d[2])) dcell = NAN;
  *dcell_out = dcell;
  if (!(dcell >= 0.0)) return false;     // error stop :510-516 (or NaN)
  return 0.0 + dcell > len;              // :421: this crossing is the segment's last
}

// ---- far.h's form (far_march's step test): the refined reciprocal and the 2^-40 margin -------
double refined_rcp(double d) {  // detmath.h ieee_rcp_f64: an approximation, two Newton steps
  double r = (double)(float)(1.0 / d);
  if (!(std::fabs(r) >= 0x1.0p-120 && std::fabs(r) <= 0x1.0p+120)) r = 1.0 / d;  // (outside fp32's range)
  double e = __builtin_fma(-d, r, 1.0);
  r = __builtin_fma(r, e, r);
  e = __builtin_fma(-d, r, 1.0);
  return __builtin_fma(r, e, r);
}
bool far_form(const double f[3], const double o[3], const double dir[3], double len) {
  bool go = len < 100000.0;
  const double lo = len * (1.0 + 0x1.0p-40);
  for (int a = 0; a < 3; ++a) {
    const bool z = dir[a] == 0.0;
    if (!(z || std::fabs(dir[a]) >= 0x1.0p-500)) return false;
    go = go && (z || (f[a] - o[a]) * refined_rcp(dir[a]) > lo);
  }
  return go;
}

bool pred(const double f[3], const double o[3], const double dir[3], double len) {
  return smcrt::invoxel_segment(o[0], o[1], o[2], dir[0], dir[1], dir[2], len, f[0], f[1], f[2]);
}

struct Grid {
  int n[3];
  double size[3];  // 2*max per axis
};
const Grid GRIDS[] = {
    {{128, 128, 128}, {2.0, 2.0, 2.0}},     // power-of-two spacing (M1)
    {{64, 32, 16}, {2.0, 4.0, 0.5}},
    {{48, 48, 48}, {2.0, 2.0, 2.0}},        // other spacings
    {{67, 67, 67}, {2.0, 2.0, 2.0}},
    {{48, 40, 56}, {0.16, 0.09, 0.13}},     // anisotropic
};
const int N_GRIDS = (int)(sizeof(GRIDS) / sizeof(GRIDS[0]));
double face_of(const Grid& g, int a, int k) { return (double)k * (g.size[a] / (double)g.n[a]); }  // face k, 0 .. n

struct Tally {
  uint64_t cases = 0, accepted = 0, violations = 0;
  uint64_t nan_true = 0, tiny_dir_true = 0, neg_num_true = 0, bad_len_true = 0;
  void print_violation(const double f[3], const double o[3], const double dir[3], double len, double dcell) {
    if (violations > 5) return;
    std::fprintf(stderr, "violation: f %a %a %a | o %a %a %a | dir %a %a %a | len %a | dcell %a\n", f[0], f[1], f[2], o[0],
                 o[1], o[2], dir[0], dir[1], dir[2], len, dcell);
  }
  void check(const double f[3], const double o[3], const double dir[3], double len) {
    ++cases;
    const bool p = pred(f, o, dir, len);
    if (!p) return;
    ++accepted;
    double dcell;
    if (!ref_single(f, o, dir, len, &dcell)) {
      ++violations;
      print_violation(f, o, dir, len, dcell);
    }
    // what must always come out false
    bool any_nan = std::isnan(len);
    for (int a = 0; a < 3; ++a) any_nan = any_nan || std::isnan(f[a]) || std::isnan(o[a]) || std::isnan(dir[a]);
    if (any_nan) ++nan_true;
    if (!(len >= 0.0 && len < 100000.0)) ++bad_len_true;
    for (int a = 0; a < 3; ++a) {
      if (dir[a] != 0.0 && std::fabs(dir[a]) < 0x1.0p-500) ++tiny_dir_true;
      const double num = f[a] - o[a];
      if ((dir[a] > 0.0 && num < 0.0) || (dir[a] < 0.0 && num > 0.0)) ++neg_num_true;
    }
  }
};

void unit_dir(Rng& r, double dir[3]) {
  for (;;) {
    const double x = r.range(-1.0, 1.0), y = r.range(-1.0, 1.0), z = r.range(-1.0, 1.0);
    const double n2 = x * x + y * y + z * z;
    if (n2 > 1.0 || n2 < 1e-6) continue;
    const double n = std::sqrt(n2);
    dir[0] = x / n; dir[1] = y / n; dir[2] = z / n;
    return;
  }
}

const double SPECIAL_DIR[] = {0.0, -0.0, 0x1.0p-500, -0x1.0p-500, 0x1.0p-501, -0x1.0p-501, 4.9406564584124654e-324,
                              -4.9406564584124654e-324, 1e-310, -1e-310, 0x1.fffffffffffffp-501, 1.0, -1.0, 1e-30, -1e-30};
const int N_SPECIAL_DIR = (int)(sizeof(SPECIAL_DIR) / sizeof(SPECIAL_DIR[0]));

// the faces wall_dist measures to from cell c (1-based): the upper one for dir > 0, else the lower
void faces_for(const Grid& g, const int c[3], const double dir[3], double f[3]) {
  for (int a = 0; a < 3; ++a) f[a] = face_of(g, a, dir[a] > 0.0 ? c[a] : c[a] - 1);
}

// one case of the given family; returns through t.check
void one_case(Rng& r, Tally& t, int family) {
  const Grid& g = GRIDS[r.below(N_GRIDS)];
  int c[3];
  double o[3], dir[3], f[3];
  for (int a = 0; a < 3; ++a) {
    c[a] = 1 + r.below(g.n[a]);
    o[a] = r.range(face_of(g, a, c[a] - 1), face_of(g, a, c[a]));
  }
  unit_dir(r, dir);
  if (family == 2 || family == 4) {  // special direction components on one to three axes
    const int k = 1 + r.below(3);
    for (int i = 0; i < k; ++i) dir[r.below(3)] = SPECIAL_DIR[r.below(N_SPECIAL_DIR)];
  }
  if (family == 1 || family == 4) {  // starts on a face, or 1-4 ulps either side of it (outside the cell too)
    const int k = 1 + r.below(3);
    for (int i = 0; i < k; ++i) {
      const int a = r.below(3);
      o[a] = ulps(face_of(g, a, c[a] - r.below(2)), r.below(9) - 4);
    }
  }
  faces_for(g, c, dir, f);
  // the length: log-uniform, or within 4 ulps of an axis's exact quotient, or a special value
  double len = std::exp(r.range(std::log(1e-9), std::log(0.2)));
  const int how = r.below(family == 3 ? 2 : 4);
  if (how == 0) {
    const int a = r.below(3);
    const double q = (f[a] - o[a]) / dir[a];
    if (std::isfinite(q)) len = ulps(q, r.below(9) - 4);
  } else if (how == 1 && family >= 3) {
    static const double SPECIAL_LEN[] = {0.0, -0.0, NAN, INFINITY, -INFINITY, -1.0, 100000.0, 0x1.869ffffffffffp+16,
                                         0x1.0p-400, 0x1.fffffffffffffp-401, 4.9406564584124654e-324, 1e-320, 1e-300};
    len = SPECIAL_LEN[r.below((int)(sizeof(SPECIAL_LEN) / sizeof(SPECIAL_LEN[0])))];
  }
  if (family == 5) {  // NaN or infinite inputs
    const double bad[] = {NAN, INFINITY, -INFINITY};
    const int where = r.below(10);
    const double b = bad[r.below(3)];
    if (where < 3) o[where] = b;
    else if (where < 6) dir[where - 3] = b;
    else if (where < 9) f[where - 6] = b;
    else len = b;
  }
  t.check(f, o, dir, len);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 4) {
    std::fprintf(stderr, "usage: invoxel_probe SEED N_RANDOM N_COMPLETE\n");
    return 2;
  }
  Rng r{std::strtoull(argv[1], nullptr, 10)};
  const uint64_t n_random = std::strtoull(argv[2], nullptr, 10), n_complete = std::strtoull(argv[3], nullptr, 10);

  // ---- soundness ----
  Tally random, adversarial;
  for (uint64_t i = 0; i < n_random; ++i) one_case(r, random, 0);
  const uint64_t n_adv = n_random / 2;
  for (int family = 1; family <= 5; ++family)
    for (uint64_t i = 0; i < n_adv / 5 + 1; ++i) one_case(r, adversarial, family);
  std::printf("random_cases=%llu\nrandom_accepted=%llu\nrandom_violations=%llu\n", (unsigned long long)random.cases,
              (unsigned long long)random.accepted, (unsigned long long)random.violations);
  std::printf("adversarial_cases=%llu\nadversarial_accepted=%llu\nadversarial_violations=%llu\n",
              (unsigned long long)adversarial.cases, (unsigned long long)adversarial.accepted,
              (unsigned long long)adversarial.violations);
  std::printf("nan_true=%llu\ntiny_dir_true=%llu\nneg_num_true=%llu\nbad_len_true=%llu\n",
              (unsigned long long)(random.nan_true + adversarial.nan_true),
              (unsigned long long)(random.tiny_dir_true + adversarial.tiny_dir_true),
              (unsigned long long)(random.neg_num_true + adversarial.neg_num_true),
              (unsigned long long)(random.bad_len_true + adversarial.bad_len_true));

  // ---- completeness: M1-like segments (128^3 over 2 x 2 x 2, starts uniform in a voxel, isotropic
  // directions, len log-uniform in [1e-8, 0.05]) ----
  uint64_t single = 0, acc_new = 0, acc_far = 0, far_only = 0, bad_new = 0, bad_far = 0;
  const Grid& g = GRIDS[0];
  for (uint64_t i = 0; i < n_complete; ++i) {
    int c[3];
    double o[3], dir[3], f[3], dcell;
    for (int a = 0; a < 3; ++a) {
      c[a] = 1 + r.below(g.n[a]);
      o[a] = r.range(face_of(g, a, c[a] - 1), face_of(g, a, c[a]));
    }
    unit_dir(r, dir);
    faces_for(g, c, dir, f);
    const double len = std::exp(r.range(std::log(1e-8), std::log(0.05)));
    const bool s = ref_single(f, o, dir, len, &dcell), pn = pred(f, o, dir, len), pf = far_form(f, o, dir, len);
    single += s;
    acc_new += s && pn;
    acc_far += s && pf;
    far_only += pf && !pn;
    bad_new += pn && !s;
    bad_far += pf && !s;
  }
  std::printf("complete_cases=%llu\ncomplete_single=%llu\ncomplete_accepted=%llu\ncomplete_accepted_far=%llu\n"
              "complete_far_only=%llu\ncomplete_violations=%llu\ncomplete_violations_far=%llu\n",
              (unsigned long long)n_complete, (unsigned long long)single, (unsigned long long)acc_new,
              (unsigned long long)acc_far, (unsigned long long)far_only, (unsigned long long)bad_new,
              (unsigned long long)bad_far);
  return 0;
}
