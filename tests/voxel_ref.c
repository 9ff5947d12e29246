/* voxel_ref.c — test infrastructure only: a serial restatement of the voxel-media semantics of
 * DESIGN.md §7 ("Voxel media"), written from that text and not from the kernel (voxel.h).
 *
 * tests/voxel_ref.py compiles it on first use with the oracle's floating-point flags
 * (-ffp-contract=off -fno-fast-math) and links it against oracle/liboracle.so, whose
 * oracle_uniform, oracle_log, oracle_sincos, oracle_reflect_refract, oracle_emit and
 * oracle_record_hit it calls. scatter, the DDA piece and the cell arithmetic are restated here
 * with the reference's expressions, as oracle/smcrt_oracle.c states them (photon.f90:1045-1103,
 * inttau2.f90:417-441, 467-614, grid.f90:51-78).
 *
 * One limit: the re-emission loop needs the photon's stream position, which oracle_emit does not
 * take. The point, uniform and pencil emitters are therefore restated here (photon.f90:311-359,
 * 566-710); a first emission of any other source that lands outside the grid returns
 * VOXEL_REF_UNSUPPORTED instead of a result. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../include/smcrt.h"

double oracle_uniform(uint64_t seed, uint64_t pid, uint32_t draw);
double oracle_log(double x);
void oracle_sincos(double x, double* s, double* c);
void oracle_reflect_refract(double I[3], const double N[3], double n1, double n2, double xi, int* rflag);
int oracle_emit(const smcrt_grid* grid, const smcrt_source* src, uint64_t seed, uint64_t first, int64_t n, double* pos,
                double* dir, int32_t* cells, uint32_t* draws);
int oracle_record_hit(const smcrt_detector* det, const double start[3], const double dir[3], double pointSep,
                      int32_t layer, double weight, double* bins, uint64_t* hits);

#define VOXEL_REF_UNSUPPORTED (-100)
/* the caps of the engine (transport.h) */
#define MAX_EMIT_TRIES 100000
#define MAX_DDA_ITERS 10000000
#define MAX_RENORM_ITERS 64
#define MAX_INTERACTIONS 100000000
#define MAX_BOUNCES 1000

typedef struct { double x, y, z; } vec3;
typedef struct { uint64_t pid, seed; uint32_t draws; } rng_t;
static double ran2(rng_t* r) { return oracle_uniform(r->seed, r->pid, r->draws++); }

typedef struct {
  const uint8_t* labels;
  int32_t n_media;
  double *kappa, *albedo, *hgg, *nidx;
  smcrt_grid grid;
  double *xface, *yface, *zface;
  const smcrt_detector* dets;
  int32_t n_dets;
  int64_t* det_off;
  uint32_t flags;
  double *jmean, *absorb, *emission, *det;
  uint64_t ctr[SMCRT_NCOUNTERS];
  double nscatt;
} ctx_t;

typedef struct {
  vec3 old;  /* the position in corner coordinates: pos + max, carried from the emission on */
  vec3 dir;
  int32_t ci, cj, ck;
  int32_t layer;  /* medium + 1 */
  uint32_t bounces, nscatt;
  double weight;
  int fault;
} packet_t;

static inline double fmind(double a, double b) { return a < b ? a : b; }
static inline double fmaxd(double a, double b) { return a > b ? a : b; }

/* update_voxels, inttau2.f90:587-614 (corner coordinates) */
static inline int32_t cell_of(double p, int32_t n, double max) {
  double f = floor(((double)n * p) / (2.0 * max));
  if (!(f >= 0.0 && f < (double)n)) return -1;
  return (int32_t)f + 1;
}
/* get_voxel_cart, grid.f90:51-78 (centred coordinates) */
static inline int32_t vox_of(double p, int32_t n, double max) {
  double f = floor(((double)n * (p + max)) / (2.0 * max));
  if (!(f >= 0.0 && f < (double)n)) return -1;
  return (int32_t)f + 1;
}
static inline int cell_out(const ctx_t* C, const packet_t* pk) {
  return pk->ci < 1 || pk->ci > C->grid.nx || pk->cj < 1 || pk->cj > C->grid.ny || pk->ck < 1 || pk->ck > C->grid.nz;
}
static inline int64_t lin(const ctx_t* C, int32_t i, int32_t j, int32_t k) {
  return (int64_t)(i - 1) + (int64_t)C->grid.nx * ((int64_t)(j - 1) + (int64_t)C->grid.ny * (int64_t)(k - 1));
}
static void add_cell(ctx_t* C, double* g, packet_t* pk, double w) {
  if (cell_out(C, pk)) { pk->fault = 1; return; }
  if (g) g[lin(C, pk->ci, pk->cj, pk->ck)] += w;
}
static double pointsep(vec3 a, vec3 b) {
  double dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;
  return sqrt(dx * dx + dy * dy + dz * dz);
}

/* record_hits once per leg: from the leg's start to where the photon stands (both centred) */
static void leg_end(ctx_t* C, const packet_t* pk, vec3 leg) {
  if (!C->n_dets) return;
  const double xm = C->grid.xmax, ym = C->grid.ymax, zm = C->grid.zmax;
  const double start[3] = {leg.x - xm, leg.y - ym, leg.z - zm};
  const vec3 s = {start[0], start[1], start[2]}, e = {pk->old.x - xm, pk->old.y - ym, pk->old.z - zm};
  const double dir[3] = {pk->dir.x, pk->dir.y, pk->dir.z};
  const double sep = pointsep(e, s);
  for (int32_t d = 0; d < C->n_dets; ++d) {
    uint64_t hits = 0;
    oracle_record_hit(C->dets + d, start, dir, sep, pk->layer, pk->weight, C->det ? C->det + C->det_off[d] : NULL, &hits);
    C->ctr[SMCRT_CTR_DETECTOR_HITS] += hits;
  }
}

/* scatter, photon.f90:1045-1103 */
static void scatter(packet_t* pk, double hgg, rng_t* rng) {
  double cost, temp;
  if (hgg == 0.0) {
    cost = 2.0 * ran2(rng) - 1.0;
  } else {
    temp = (1.0 - hgg * hgg) / (1.0 - hgg + 2.0 * hgg * ran2(rng));
    cost = (1.0 + hgg * hgg - temp * temp) / (2.0 * hgg);
  }
  double sint = sqrt(1.0 - cost * cost);
  double phi = 6.283185307179586 * ran2(rng);
  double sinp, cosp;
  oracle_sincos(phi, &sinp, &cosp);
  double nxp = pk->dir.x, nyp = pk->dir.y, nzp = pk->dir.z, uxx, uyy, uzz;
  if (nzp > 1.0 - 1e-12) {
    uxx = sint * cosp; uyy = sint * sinp; uzz = cost;
  } else if (nzp < -1.0 + 1e-12) {
    uxx = sint * cosp; uyy = sint * sinp; uzz = -cost;
  } else {
    temp = sqrt(1.0 - nzp * nzp);
    uxx = sint * ((nxp * nzp * cosp - nyp * sinp) / temp) + nxp * cost;
    uyy = sint * ((nyp * nzp * cosp + nxp * sinp) / temp) + nyp * cost;
    uzz = -1.0 * sint * cosp * temp + nzp * cost;
  }
  temp = sqrt(uxx * uxx + uyy * uyy + uzz * uzz);
  int it = 0;
  while (fabs(temp - 1.0) > 1e-12) {
    if (++it > MAX_RENORM_ITERS) { pk->fault = 1; break; }
    uxx = uxx / temp; uyy = uyy / temp; uzz = uzz / temp;
    temp = sqrt(uxx * uxx + uyy * uyy + uzz * uzz);
  }
  pk->dir.x = uxx; pk->dir.y = uyy; pk->dir.z = uzz;
}

/* One emission. Returns 0, or VOXEL_REF_UNSUPPORTED for a re-emission of a general source. */
static int emit(ctx_t* C, const smcrt_source* src, packet_t* pk, rng_t* rng, int again) {
  const double xmax = C->grid.xmax, ymax = C->grid.ymax, zmax = C->grid.zmax;
  vec3 pos;
  const int plain = src->kind <= SMCRT_SRC_PENCIL && !(src->spectrum && src->spectrum->kind != SMCRT_SPEC_CONSTANT);
  if (!plain) {
    if (again) return VOXEL_REF_UNSUPPORTED;
    double p[3], d[3];
    int32_t cells[3];
    uint32_t draws = 0;
    int st = oracle_emit(&C->grid, src, rng->seed, rng->pid, 1, p, d, cells, &draws);
    if (st) return st;
    rng->draws += draws;
    pos.x = p[0]; pos.y = p[1]; pos.z = p[2];
    pk->dir.x = d[0]; pk->dir.y = d[1]; pk->dir.z = d[2];
  } else if (src->kind == SMCRT_SRC_POINT) {                         /* photon.f90:311-359 */
    pos.x = src->pos[0]; pos.y = src->pos[1]; pos.z = src->pos[2];
    double phi = ran2(rng) * 6.283185307179586;
    double sinp, cosp;
    oracle_sincos(phi, &sinp, &cosp);
    double cost = 2.0 * ran2(rng) - 1.0;
    double sint = sqrt(1.0 - cost * cost);
    pk->dir.x = sint * cosp; pk->dir.y = sint * sinp; pk->dir.z = cost;
  } else {
    if (src->kind == SMCRT_SRC_UNIFORM) {                            /* :566-649 */
      double rx = ran2(rng), ry = ran2(rng);
      pos.x = src->p1[0] + rx * src->p2[0] + ry * src->p3[0];
      pos.y = src->p1[1] + rx * src->p2[1] + ry * src->p3[1];
      pos.z = src->p1[2] + rx * src->p2[2] + ry * src->p3[2];
    } else {                                                         /* pencil :652-710 */
      pos.x = src->pos[0]; pos.y = src->pos[1]; pos.z = src->pos[2];
    }
    if (pos.x == -xmax) pos.x = pos.x + 7.9e-7;
    else if (pos.x == xmax) pos.x = pos.x - 7.9e-7;
    if (pos.y == -ymax) pos.y = pos.y + 7.9e-7;
    else if (pos.y == ymax) pos.y = pos.y - 7.9e-7;
    if (pos.z == -zmax) pos.z = pos.z + 7.9e-7;
    else if (pos.z == zmax) pos.z = pos.z - 7.9e-7;
    pk->dir.x = src->dir[0]; pk->dir.y = src->dir[1]; pk->dir.z = src->dir[2];
  }
  pk->weight = 1.0;
  pk->ci = vox_of(pos.x, C->grid.nx, xmax);
  pk->cj = vox_of(pos.y, C->grid.ny, ymax);
  pk->ck = vox_of(pos.z, C->grid.nz, zmax);
  pk->old.x = pos.x + xmax; pk->old.y = pos.y + ymax; pk->old.z = pos.z + zmax;
  return 0;
}

enum { END_INTERACT = 0, END_ESCAPED = 1, END_FAULT = 2 };

/* One flight: pieces until the optical depth is used up inside a voxel, the photon leaves the
 * grid, or a fault. */
static int flight(ctx_t* C, packet_t* pk, rng_t* rng) {
  const double delta = 1e-8;                                         /* inttau2.f90:393 */
  C->ctr[SMCRT_CTR_TAUINT]++;
  double tau_left = -oracle_log(ran2(rng));
  pk->bounces = 0;
  vec3 leg = pk->old;
  C->ctr[SMCRT_CTR_GRID_UPDATES]++;
  for (int64_t it = 0;; ++it) {
    if (it >= MAX_DDA_ITERS) { pk->fault = 1; return END_FAULT; }
    const int32_t m = pk->layer - 1;
    const double kappa = C->kappa[m];
    const double s_max = kappa > 0.0 ? tau_left / kappa : HUGE_VAL;
    const vec3 dir = pk->dir;
    vec3 old = pk->old;
    int32_t ci = pk->ci, cj = pk->cj, ck = pk->ck;
    /* wall_dist, inttau2.f90:467-521 */
    double dx = -999.0, dy = -999.0, dz = -999.0;
    if (dir.x > 0.0) dx = (C->xface[ci] - old.x) / dir.x;
    else if (dir.x < 0.0) dx = (C->xface[ci - 1] - old.x) / dir.x;
    else if (dir.x == 0.0) dx = 100000.0;
    if (dir.y > 0.0) dy = (C->yface[cj] - old.y) / dir.y;
    else if (dir.y < 0.0) dy = (C->yface[cj - 1] - old.y) / dir.y;
    else if (dir.y == 0.0) dy = 100000.0;
    if (dir.z > 0.0) dz = (C->zface[ck] - old.z) / dir.z;
    else if (dir.z < 0.0) dz = (C->zface[ck - 1] - old.z) / dir.z;
    else if (dir.z == 0.0) dz = 100000.0;
    double dcell = fmind(fmind(dx, dy), dz);
    if (dcell < 0.0) { pk->fault = 1; return END_FAULT; }            /* error stop :510-516: it ends where it stood */
    const int lx = (dcell == dx), ly = (dcell == dy), lz = (dcell == dz);
    const int last = 0.0 + dcell > s_max;                            /* :421 with d = 0 */
    if (last) dcell = s_max - 0.0;
    if (C->flags & SMCRT_FLAG_PATHLENGTH) {                          /* :427 / :434, into the voxel being left */
      C->ctr[SMCRT_CTR_DEPOSITS]++;
      if (C->jmean) C->jmean[lin(C, ci, cj, ck)] += (double)(float)dcell * pk->weight;
    }
    if (last) {                                                      /* update_pos(.false.) */
      old.x = old.x + dir.x * dcell;
      old.y = old.y + dir.y * dcell;
      old.z = old.z + dir.z * dcell;
      pk->old = old;
      leg_end(C, pk, leg);
      return END_INTERACT;                                           /* tau_left = 0 */
    }
    /* update_pos(.true.), :538-582 */
    int axis;
    double wall = 0.0, sdelta = 0.0;
    if (lx) {
      axis = 0;
      if (dir.x > 0.0) { wall = C->xface[ci]; sdelta = delta; old.x = wall + delta; }
      else if (dir.x < 0.0) { wall = C->xface[ci - 1]; sdelta = -delta; old.x = wall - delta; }
      else { wall = C->xface[ci - 1]; sdelta = -delta; }  /* (a still axis keeps its coordinate; named as if moving down) */
      old.y = old.y + dir.y * dcell;
      old.z = old.z + dir.z * dcell;
    } else if (ly) {
      axis = 1;
      if (dir.y > 0.0) { wall = C->yface[cj]; sdelta = delta; old.y = wall + delta; }
      else if (dir.y < 0.0) { wall = C->yface[cj - 1]; sdelta = -delta; old.y = wall - delta; }
      else { wall = C->yface[cj - 1]; sdelta = -delta; }  /* (a still axis keeps its coordinate; named as if moving down) */
      old.x = old.x + dir.x * dcell;
      old.z = old.z + dir.z * dcell;
    } else if (lz) {
      axis = 2;
      if (dir.z > 0.0) { wall = C->zface[ck]; sdelta = delta; old.z = wall + delta; }
      else if (dir.z < 0.0) { wall = C->zface[ck - 1]; sdelta = -delta; old.z = wall - delta; }
      else { wall = C->zface[ck - 1]; sdelta = -delta; }  /* (a still axis keeps its coordinate; named as if moving down) */
      old.x = old.x + dir.x * dcell;
      old.y = old.y + dir.y * dcell;
    } else {                                                         /* error stop :570-573 */
      pk->fault = 1;
      return END_FAULT;
    }
    tau_left = fmaxd(tau_left - kappa * dcell, 0.0);
    const int32_t pi = ci, pj = cj, pk_ = ck;
    ci = cell_of(old.x, C->grid.nx, C->grid.xmax);                   /* update_voxels */
    cj = cell_of(old.y, C->grid.ny, C->grid.ymax);
    ck = cell_of(old.z, C->grid.nz, C->grid.zmax);
    pk->old = old; pk->ci = ci; pk->cj = cj; pk->ck = ck;
    if (ci == -1 || cj == -1 || ck == -1) {                          /* the world ends at the grid */
      leg_end(C, pk, leg);
      return END_ESCAPED;
    }
    const int32_t m2 = C->labels[lin(C, ci, cj, ck)];
    if (m2 == m) continue;
    if (C->nidx[m2] == C->nidx[m]) { pk->layer = m2 + 1; continue; }  /* no draw, the leg continues */
    /* an interface: the leg ends, one draw, reflect or refract at the wall's normal */
    leg_end(C, pk, leg);
    C->ctr[SMCRT_CTR_FRESNEL]++;
    double I[3] = {dir.x, dir.y, dir.z}, N[3] = {0.0, 0.0, 0.0};
    N[axis] = sdelta > 0.0 ? 1.0 : -1.0;                             /* outward normal of the voxel being left */
    int rflag = 0;
    oracle_reflect_refract(I, N, C->nidx[m], C->nidx[m2], ran2(rng), &rflag);
    pk->dir.x = I[0]; pk->dir.y = I[1]; pk->dir.z = I[2];
    if (rflag) {
      /* back on the side it came from; the crossed axis' cell index goes back */
      if (axis == 0) { pk->old.x = wall - sdelta; pk->ci = pi; }
      else if (axis == 1) { pk->old.y = wall - sdelta; pk->cj = pj; }
      else { pk->old.z = wall - sdelta; pk->ck = pk_; }
      C->ctr[SMCRT_CTR_REFLECTIONS]++;
      pk->bounces += 1;
      if (pk->bounces > MAX_BOUNCES) {
        C->ctr[SMCRT_CTR_BOUNCE_ABORTS]++;
        pk->fault = 1;
        return END_FAULT;
      }
    } else {
      pk->layer = m2 + 1;
    }
    leg = pk->old;
    C->ctr[SMCRT_CTR_GRID_UPDATES]++;
  }
}

static int run_photon(ctx_t* C, const smcrt_source* src, uint64_t pid, uint64_t seed, smcrt_photon_record* rec) {
  rng_t rng = {pid, seed, 0};
  packet_t pk;
  memset(&pk, 0, sizeof pk);
  uint32_t status = 0;
  int st = emit(C, src, &pk, &rng, 0);
  if (st) return st;
  int tries = 0;
  while (cell_out(C, &pk)) {
    if (++tries > MAX_EMIT_TRIES) { pk.fault = 1; break; }
    C->ctr[SMCRT_CTR_EMIT_RETRIES]++;
    if ((st = emit(C, src, &pk, &rng, 1))) return st;
  }
  if (!pk.fault) {
    if (C->flags & SMCRT_FLAG_RENDER_SOURCE) add_cell(C, C->emission, &pk, 1.0);
    pk.layer = (int32_t)C->labels[lin(C, pk.ci, pk.cj, pk.ck)] + 1;
    uint64_t inter = 0;
    int end = flight(C, &pk, &rng);
    while (end == END_INTERACT && !pk.fault) {
      if (++inter > MAX_INTERACTIONS) { pk.fault = 1; break; }
      const double ran = ran2(&rng);
      const int32_t m = pk.layer - 1;
      if (C->flags & SMCRT_FLAG_SURVIVAL_BIAS) {                     /* kernelsMod.f90:2041-2062 */
        const double w_abs = pk.weight * (1.0 - C->albedo[m]);
        pk.weight = pk.weight - w_abs;
        add_cell(C, C->absorb, &pk, w_abs);
        if (pk.weight < 0.01) {
          if (ran < 0.1) {
            pk.weight = pk.weight / 0.1;
          } else {
            status = 1;
            C->ctr[SMCRT_CTR_ABSORBED]++;
            break;
          }
        }
      } else if (!(ran < C->albedo[m])) {                            /* :1958-1975 */
        status = 1;
        C->ctr[SMCRT_CTR_ABSORBED]++;
        add_cell(C, C->absorb, &pk, 1.0);
        break;
      }
      scatter(&pk, C->hgg[m], &rng);
      pk.nscatt++;
      C->nscatt += 1.0;
      C->ctr[SMCRT_CTR_SCATTERS]++;
      if (pk.fault) break;
      end = flight(C, &pk, &rng);
    }
  }
  if (pk.fault) { status = 3; C->ctr[SMCRT_CTR_FAULTS]++; }
  else if (status == 0) { status = 2; C->ctr[SMCRT_CTR_ESCAPED]++; }
  C->ctr[SMCRT_CTR_PHOTONS]++;
  C->ctr[SMCRT_CTR_RNG_DRAWS] += rng.draws;
  if (rec) {
    rec->pos[0] = pk.old.x - C->grid.xmax; rec->pos[1] = pk.old.y - C->grid.ymax; rec->pos[2] = pk.old.z - C->grid.zmax;
    rec->dir[0] = pk.dir.x; rec->dir[1] = pk.dir.y; rec->dir[2] = pk.dir.z;
    rec->weight = pk.weight;
    rec->cell[0] = pk.ci; rec->cell[1] = pk.cj; rec->cell[2] = pk.ck;
    rec->layer = pk.layer;
    rec->nscatt = pk.nscatt;
    rec->bounces = pk.bounces;
    rec->draws = rng.draws;
    rec->status = status;
  }
  return 0;
}

/* The photon loop (serial, photon order), accumulating into the fp64 fields of `io`. */
int voxel_ref_run(const uint8_t* labels, const smcrt_medium* media, int32_t n_media, const smcrt_grid* grid,
                  const smcrt_detector* dets, int32_t n_dets, const smcrt_source* src, const smcrt_run_config* cfg,
                  smcrt_tallies* io) {
  if (!labels || !media || n_media < 1 || n_media > 256 || !grid || !src || !cfg || !io) return SMCRT_ERR_INVALID_ARG;
  if (cfg->flags & (SMCRT_FLAG_TEST_KERNEL | SMCRT_FLAG_END_EARLY | SMCRT_FLAG_TRACK_PATHS | SMCRT_FLAG_PHASOR))
    return SMCRT_ERR_UNSUPPORTED;
  ctx_t C;
  memset(&C, 0, sizeof C);
  C.labels = labels; C.n_media = n_media; C.grid = *grid; C.dets = dets; C.n_dets = n_dets; C.flags = cfg->flags;
  C.kappa = calloc(4 * (size_t)n_media, sizeof(double));
  C.albedo = C.kappa + n_media; C.hgg = C.albedo + n_media; C.nidx = C.hgg + n_media;
  for (int32_t i = 0; i < n_media; ++i) {                            /* init_mono, opticalProperties.f90:107-125 */
    C.kappa[i] = media[i].mus + media[i].mua;
    C.albedo[i] = (media[i].mua < 1e-9) ? 1.0 : media[i].mus / C.kappa[i];
    C.hgg[i] = media[i].hgg; C.nidx[i] = media[i].n;
  }
  C.xface = calloc((size_t)grid->nx + 1 + grid->ny + 1 + grid->nz + 2, sizeof(double));
  C.yface = C.xface + grid->nx + 1;
  C.zface = C.yface + grid->ny + 1;
  for (int32_t i = 0; i < grid->nx + 1; ++i) C.xface[i] = (double)i * 2.0 * grid->xmax / (double)grid->nx;  /* grid.f90:147-157 */
  for (int32_t i = 0; i < grid->ny + 1; ++i) C.yface[i] = (double)i * 2.0 * grid->ymax / (double)grid->ny;
  for (int32_t i = 0; i < grid->nz + 2; ++i) C.zface[i] = (double)i * 2.0 * grid->zmax / (double)grid->nz;
  C.det_off = calloc((size_t)n_dets + 1, sizeof(int64_t));
  for (int32_t i = 0; i < n_dets; ++i) {
    int64_t nb = dets[i].nbins;
    C.det_off[i + 1] = C.det_off[i] + (dets[i].kind == SMCRT_DET_CAMERA ? nb * nb : nb);
  }
  C.jmean = io->jmean_f64; C.absorb = io->absorb_f64; C.emission = io->emission_f64; C.det = io->det_bins;
  int st = 0;
  for (uint64_t j = 0; j < cfg->n_photons && !st; ++j) {
    smcrt_photon_record* rec = (io->records && (cfg->flags & SMCRT_FLAG_RECORD_PHOTONS)) ? &io->records[j] : NULL;
    st = run_photon(&C, src, cfg->first_photon + j, cfg->seed, rec);
  }
  if (io->nscatt) *io->nscatt += C.nscatt;
  if (io->counters)
    for (int i = 0; i < SMCRT_NCOUNTERS; ++i) io->counters[i] += C.ctr[i];
  free(C.kappa); free(C.xface); free(C.det_off);
  return st;
}
