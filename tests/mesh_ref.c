/* mesh_ref.c — test infrastructure only: a serial restatement of the mesh-media semantics of
 * DESIGN.md §7 ("Mesh media"), written from that text and not from the kernel (mesh.h).
 *
 * tests/mesh_ref.py compiles it on first use with the oracle's floating-point flags
 * (-ffp-contract=off -fno-fast-math) and links it against oracle/liboracle.so, as voxel_ref.c is
 * built; scatter, the emitters, the DDA pieces and the cell arithmetic are restated as there.
 *
 * The cast is the definition itself: a loop over ALL triangles in index order with the
 * Moeller-Trumbore test of DESIGN.md, keeping the smallest t > 0 (the first of equal ones). No
 * bounding-volume hierarchy is built here. mesh_ref_cast exposes it to the tests. */
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

#define MESH_REF_UNSUPPORTED (-100)
/* the caps of the engine (transport.h) */
#define MAX_EMIT_TRIES 100000
#define MAX_DDA_ITERS 10000000
#define MAX_RENORM_ITERS 64
#define MAX_INTERACTIONS 100000000
#define MAX_BOUNCES 1000
#define MAX_HOP_ITERS 1000000
#define MESH_NONE (-1)

typedef struct { double x, y, z; } vec3;
typedef struct { uint64_t pid, seed; uint32_t draws; } rng_t;
static double ran2(rng_t* r) { return oracle_uniform(r->seed, r->pid, r->draws++); }

typedef struct {
  vec3 v0, e1, e2, N;
  int32_t outside, inside;
} tri_t;

typedef struct {
  const tri_t* tris;
  int32_t nt, ambient;
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
  vec3 pos;  /* the position in centred coordinates */
  vec3 old;  /* the walk's position in corner coordinates, set by each leg */
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

/* record_hits once per leg: from the leg's start to its end (both centred); skipped when the
 * separation is not finite (a leg to infinity that was jumped, not walked) */
static void leg_end(ctx_t* C, const packet_t* pk, vec3 s, vec3 e) {
  if (!C->n_dets) return;
  const double start[3] = {s.x, s.y, s.z};
  const double dir[3] = {pk->dir.x, pk->dir.y, pk->dir.z};
  const double sep = pointsep(e, s);
  if (!(sep < HUGE_VAL)) return;
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

/* One emission. Returns 0, or MESH_REF_UNSUPPORTED for a re-emission of a general source. */
static int emit(ctx_t* C, const smcrt_source* src, packet_t* pk, rng_t* rng, int again) {
  const double xmax = C->grid.xmax, ymax = C->grid.ymax, zmax = C->grid.zmax;
  vec3 pos;
  const int plain = src->kind <= SMCRT_SRC_PENCIL && !(src->spectrum && src->spectrum->kind != SMCRT_SPEC_CONSTANT);
  if (!plain) {
    if (again) return MESH_REF_UNSUPPORTED;
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
  pk->pos = pos;
  return 0;
}


static inline vec3 vsub3(vec3 a, vec3 b) { vec3 r = {a.x - b.x, a.y - b.y, a.z - b.z}; return r; }
static inline vec3 cross3(vec3 a, vec3 b) {
  vec3 r = {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
  return r;
}
static inline double dot3(vec3 a, vec3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }

static void make_tris(const double* verts, const int32_t* tris, const uint8_t* tri_media, int32_t nt, tri_t* out) {
  for (int32_t t = 0; t < nt; ++t) {
    const double *a = verts + 3 * (size_t)tris[3 * t], *b = verts + 3 * (size_t)tris[3 * t + 1],
                 *c = verts + 3 * (size_t)tris[3 * t + 2];
    tri_t* T = out + t;
    T->v0.x = a[0]; T->v0.y = a[1]; T->v0.z = a[2];
    T->e1.x = b[0] - a[0]; T->e1.y = b[1] - a[1]; T->e1.z = b[2] - a[2];
    T->e2.x = c[0] - a[0]; T->e2.y = c[1] - a[1]; T->e2.z = c[2] - a[2];
    const vec3 n = cross3(T->e1, T->e2);
    const double len = sqrt(n.x * n.x + n.y * n.y + n.z * n.z);
    T->N.x = n.x / len; T->N.y = n.y / len; T->N.z = n.z / len;
    T->outside = tri_media ? tri_media[2 * t] : 0;
    T->inside = tri_media ? tri_media[2 * t + 1] : 0;
  }
}

/* DESIGN.md §7, the per-triangle test, in its order of operations */
static int tri_test(const tri_t* T, vec3 o, vec3 dir, double* t) {
  const vec3 p = cross3(dir, T->e2);
  const double det = dot3(T->e1, p);
  if (det == 0.0) return 0;
  const double inv = 1.0 / det;
  const vec3 s = vsub3(o, T->v0);
  const double u = dot3(s, p) * inv;
  if (u < 0.0 || u > 1.0) return 0;
  const vec3 q = cross3(s, T->e1);
  const double v = dot3(dir, q) * inv;
  if (v < 0.0 || u + v > 1.0) return 0;
  *t = dot3(T->e2, q) * inv;
  return *t > 0.0;
}

/* cast(o, dir, skip): the smallest t > 0 over all triangles != skip, ties to the smallest index */
static int32_t cast(const tri_t* tris, int32_t nt, vec3 o, vec3 dir, int32_t skip, double* t_hit) {
  int32_t best = MESH_NONE;
  double tb = HUGE_VAL;
  for (int32_t i = 0; i < nt; ++i) {
    double t;
    if (i != skip && tri_test(tris + i, o, dir, &t) && t < tb) { tb = t; best = i; }
  }
  *t_hit = tb;
  return best;
}

int mesh_ref_cast(const double* verts, const int32_t* tris, int32_t nt, int64_t n_rays, const double* origins,
                  const double* dirs, const int32_t* skips, double* t_out, int32_t* tri_out) {
  tri_t* T = malloc(sizeof(tri_t) * (size_t)nt);
  if (!T) return SMCRT_ERR_INVALID_ARG;
  make_tris(verts, tris, NULL, nt, T);
  for (int64_t r = 0; r < n_rays; ++r) {
    const vec3 o = {origins[3 * r], origins[3 * r + 1], origins[3 * r + 2]}, d = {dirs[3 * r], dirs[3 * r + 1], dirs[3 * r + 2]};
    tri_out[r] = cast(T, nt, o, d, skips ? skips[r] : MESH_NONE, t_out + r);
  }
  free(T);
  return 0;
}

enum { LEG_DONE = 0, LEG_ESCAPED = 1, LEG_FAULT = 2 };

/* One leg: start_segment(pos, dlen) and its dda_step pieces (update_grids, inttau2.f90:367-584, as
 * oracle/smcrt_oracle.c states it), then pos = pos + dir * dlen. Detectors once, from the leg's
 * start to where the photon stands. */
static int leg(ctx_t* C, packet_t* pk, double dlen) {
  const double xmax = C->grid.xmax, ymax = C->grid.ymax, zmax = C->grid.zmax;
  const double delta = 1e-8;                                         /* inttau2.f90:393 */
  const vec3 dir = pk->dir, start = pk->pos;
  C->ctr[SMCRT_CTR_GRID_UPDATES]++;
  vec3 old = {start.x + xmax, start.y + ymax, start.z + zmax};
  int32_t ci = cell_of(old.x, C->grid.nx, xmax), cj = cell_of(old.y, C->grid.ny, ymax), ck = cell_of(old.z, C->grid.nz, zmax);
  pk->ci = ci; pk->cj = cj; pk->ck = ck;
  int tflag = 0;
  const vec3 jump = {start.x + dir.x * dlen, start.y + dir.y * dlen, start.z + dir.z * dlen};
  if (!(C->flags & SMCRT_FLAG_PATHLENGTH)) {                         /* :446-463 */
    old.x = old.x + dir.x * dlen;
    old.y = old.y + dir.y * dlen;
    old.z = old.z + dir.z * dlen;
    ci = cell_of(old.x, C->grid.nx, xmax); cj = cell_of(old.y, C->grid.ny, ymax); ck = cell_of(old.z, C->grid.nz, zmax);
    pk->ci = ci; pk->cj = cj; pk->ck = ck;
    tflag = (ci == -1 || cj == -1 || ck == -1);
    leg_end(C, pk, start, jump);
    pk->pos = jump;
    return tflag ? LEG_ESCAPED : LEG_DONE;
  }
  if (ci == -1 || cj == -1 || ck == -1) {                            /* :411-415 */
    tflag = 1;
  } else {
    double d = 0.0;
    for (int64_t it = 0;; ++it) {
      if (it >= MAX_DDA_ITERS) { pk->fault = 1; return LEG_FAULT; }
      double dx = -999.0, dy = -999.0, dz = -999.0;                  /* wall_dist, :467-521 */
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
      if (dcell < 0.0) { pk->fault = 1; return LEG_FAULT; }          /* error stop :510-516 */
      const int lx = (dcell == dx), ly = (dcell == dy), lz = (dcell == dz);
      const int last = d + dcell > dlen;                             /* :421-429 */
      if (last) dcell = dlen - d;
      C->ctr[SMCRT_CTR_DEPOSITS]++;
      if (C->jmean) C->jmean[lin(C, ci, cj, ck)] += (double)(float)dcell * pk->weight;
      if (last) break;                                               /* (the walk's own position is dead) */
      d = d + dcell;
      if (lx) {                                                      /* update_pos(.true.), :538-582 */
        if (dir.x > 0.0) old.x = C->xface[ci] + delta;
        else if (dir.x < 0.0) old.x = C->xface[ci - 1] - delta;
        old.y = old.y + dir.y * dcell;
        old.z = old.z + dir.z * dcell;
      } else if (ly) {
        if (dir.y > 0.0) old.y = C->yface[cj] + delta;
        else if (dir.y < 0.0) old.y = C->yface[cj - 1] - delta;
        old.x = old.x + dir.x * dcell;
        old.z = old.z + dir.z * dcell;
      } else if (lz) {
        if (dir.z > 0.0) old.z = C->zface[ck] + delta;
        else if (dir.z < 0.0) old.z = C->zface[ck - 1] - delta;
        old.x = old.x + dir.x * dcell;
        old.y = old.y + dir.y * dcell;
      } else {                                                       /* error stop :570-573 */
        pk->fault = 1;
        return LEG_FAULT;
      }
      ci = cell_of(old.x, C->grid.nx, xmax); cj = cell_of(old.y, C->grid.ny, ymax); ck = cell_of(old.z, C->grid.nz, zmax);
      pk->ci = ci; pk->cj = cj; pk->ck = ck;
      if (ci == -1 || cj == -1 || ck == -1) { tflag = 1; break; }    /* :437-440 */
    }
  }
  if (tflag) {  /* escaped: it stands where the walk stood */
    const vec3 end = {old.x - xmax, old.y - ymax, old.z - zmax};
    leg_end(C, pk, start, end);
    pk->pos = end;
    return LEG_ESCAPED;
  }
  leg_end(C, pk, start, jump);
  pk->pos = jump;
  return LEG_DONE;
}

enum { END_INTERACT = 0, END_ESCAPED = 1, END_FAULT = 2 };

/* One flight: legs until one ends inside a medium, the photon leaves the grid, or a fault.
 * `fresh`: the photon's medium comes from the first cast (emission rule). */
static int flight(ctx_t* C, packet_t* pk, rng_t* rng, int fresh) {
  C->ctr[SMCRT_CTR_TAUINT]++;
  double tau_left = -oracle_log(ran2(rng));
  pk->bounces = 0;
  int32_t skip = MESH_NONE;
  for (int64_t legs = 1;; ++legs) {
    if (legs > MAX_HOP_ITERS) { pk->fault = 1; return END_FAULT; }
    double t_hit;
    const int32_t f = cast(C->tris, C->nt, pk->pos, pk->dir, skip, &t_hit);
    if (fresh) {
      fresh = 0;
      int32_t m0 = C->ambient;
      if (f != MESH_NONE) m0 = dot3(pk->dir, C->tris[f].N) > 0.0 ? C->tris[f].inside : C->tris[f].outside;
      pk->layer = m0 + 1;
    }
    const int32_t m = pk->layer - 1;
    const double kappa = C->kappa[m];
    const double s_max = kappa > 0.0 ? tau_left / kappa : HUGE_VAL;
    const int surf = f != MESH_NONE && !(s_max < t_hit);
    const double dlen = surf ? t_hit : s_max;
    const int end = leg(C, pk, dlen);
    if (end == LEG_FAULT) return END_FAULT;
    if (end == LEG_ESCAPED) return END_ESCAPED;
    if (!surf) return END_INTERACT;                                  /* tau_left = 0 */
    const tri_t* T = C->tris + f;
    tau_left = fmaxd(tau_left - kappa * t_hit, 0.0);
    const int entering = dot3(pk->dir, T->N) < 0.0;
    const int32_t expect = entering ? T->outside : T->inside, m2 = entering ? T->inside : T->outside;
    skip = f;
    if (m != expect) { pk->fault = 1; return END_FAULT; }            /* a leaky or intersecting mesh, a crack */
    if (C->nidx[m2] == C->nidx[m]) { pk->layer = m2 + 1; continue; } /* no draw */
    C->ctr[SMCRT_CTR_FRESNEL]++;
    double I[3] = {pk->dir.x, pk->dir.y, pk->dir.z};
    const double N[3] = {T->N.x, T->N.y, T->N.z};
    int rflag = 0;
    oracle_reflect_refract(I, N, C->nidx[m], C->nidx[m2], ran2(rng), &rflag);
    pk->dir.x = I[0]; pk->dir.y = I[1]; pk->dir.z = I[2];
    if (rflag) {
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
    uint64_t inter = 0;
    int end = flight(C, &pk, &rng, 1);
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
      end = flight(C, &pk, &rng, 0);
    }
  }
  if (pk.fault) { status = 3; C->ctr[SMCRT_CTR_FAULTS]++; }
  else if (status == 0) { status = 2; C->ctr[SMCRT_CTR_ESCAPED]++; }
  C->ctr[SMCRT_CTR_PHOTONS]++;
  C->ctr[SMCRT_CTR_RNG_DRAWS] += rng.draws;
  if (rec) {
    rec->pos[0] = pk.pos.x; rec->pos[1] = pk.pos.y; rec->pos[2] = pk.pos.z;
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

/* The photon loop (serial, photon order), accumulating into the fp64 fields of `io`. The mesh is
 * taken as valid (smcrt_mesh_scene_create's checks are not restated). */
int mesh_ref_run(const double* verts, int32_t nv, const int32_t* tris, const uint8_t* tri_media, int32_t nt,
                 const smcrt_medium* media, int32_t n_media, int32_t ambient, const smcrt_grid* grid,
                 const smcrt_detector* dets, int32_t n_dets, const smcrt_source* src, const smcrt_run_config* cfg,
                 smcrt_tallies* io) {
  if (!verts || nv < 1 || !tris || !tri_media || nt < 1 || !media || n_media < 1 || n_media > 256 || ambient < 0 ||
      ambient >= n_media || !grid || !src || !cfg || !io)
    return SMCRT_ERR_INVALID_ARG;
  if (cfg->flags & (SMCRT_FLAG_TEST_KERNEL | SMCRT_FLAG_END_EARLY | SMCRT_FLAG_TRACK_PATHS | SMCRT_FLAG_PHASOR))
    return SMCRT_ERR_UNSUPPORTED;
  ctx_t C;
  memset(&C, 0, sizeof C);
  tri_t* T = malloc(sizeof(tri_t) * (size_t)nt);
  make_tris(verts, tris, tri_media, nt, T);
  C.tris = T; C.nt = nt; C.ambient = ambient;
  C.n_media = n_media; C.grid = *grid; C.dets = dets; C.n_dets = n_dets; C.flags = cfg->flags;
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
  free(C.kappa); free(C.xface); free(C.det_off); free(T);
  return st;
}
