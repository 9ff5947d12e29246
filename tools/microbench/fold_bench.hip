// Microbenchmark and exactness check of the bucketed deposit fold on its own (deposit.h: bk_scan,
// bk_place, bk_reduce, launched as enqueue_fold launches them), without a transport kernel.
// A synthetic pool: `tiles` tiles, `buckets` buckets per tile with `fill` records each, ids dealt
// to the tiles in turn (as the persistent blocks' claims interleave), voxels random within the tile.
// Question: how many records per CU-cycle does bk_reduce sum, with the whole chip (HBM-fed) and
// on 32 blocks (the regime of the bench, where the fold only gets the few CUs a transport launch
// has left), against the 2.36 fp64 LDS adds per CU-cycle of lds_atomic_bench?
//   fold_bench [--tiles T] [--buckets B] [--fill F]    timing
//   fold_bench --check                                 jmean bit for bit against a host sum
// --check uses small integer values, whose fp64 sums are exact in any order: every bucket count
// per tile in 0..130 (and tiles split into several pieces), the fills 1, 2, 3, 4, 5, 63, 64, 65,
// 255, 256 and all of them mixed, retired ids in between, a last tile cut by n_voxels.
// Build (from the repository root):
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off tools/microbench/fold_bench.hip -o tools/microbench/fold_bench
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#define SMCRT_FOLD_KERNELS
#include "../../include/smcrt.h"
#include "../../rsmcrt_amd/csrc/scene_internal.h"
#include "../../rsmcrt_amd/csrc/transport.h"
#include "../../rsmcrt_amd/csrc/deposit.h"

using namespace smcrt;

#define CHECK(x) do { hipError_t e = (x); if (e != hipSuccess) { \
  printf("HIP error %s at %s:%d\n", hipGetErrorString(e), __FILE__, __LINE__); return 1; } } while (0)

__host__ __device__ inline uint32_t hash32(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16; return x;
}
// record `slot` of bucket `id`: its voxel within a tile of `span` voxels and its value (1..16)
__host__ __device__ inline uint32_t rec_vox(uint32_t id, uint32_t slot, uint32_t span) {
  return hash32(id * BUCKET_RECORDS + slot) % span;
}
__host__ __device__ inline float rec_val(uint32_t id, uint32_t slot) {
  return (float)(1u + (hash32(0x9e3779b9u ^ (id * BUCKET_RECORDS + slot)) & 15u));
}

// One thread per record slot of the pool. Slots at and past the bucket's fill get a value and a
// voxel that a sum would show (the fold must not read them into jmean).
__global__ void fill_pool(unsigned long long* pool, const uint32_t* bucket_tile, const uint32_t* bucket_fill,
                          uint32_t n_buckets, uint32_t n_tiles, uint64_t n_voxels) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t id = (uint32_t)(i >> BUCKET_SHIFT), slot = (uint32_t)i & (BUCKET_RECORDS - 1);
  if (id >= n_buckets) return;
  const uint32_t t = bucket_tile[id];
  uint32_t span = TILE_VOXELS;
  if (t < n_tiles && ((uint64_t)t + 1) * TILE_VOXELS > n_voxels) span = (uint32_t)(n_voxels - (uint64_t)t * TILE_VOXELS);
  const bool live = t < n_tiles && slot < bucket_fill[id];
  uint32_t* const bv = (uint32_t*)(pool + ((uint64_t)id << BUCKET_SHIFT));
  bv[slot] = __float_as_uint(live ? rec_val(id, slot) : 1.0e30f);
  ((uint16_t*)(bv + BUCKET_RECORDS))[slot] = live ? (uint16_t)rec_vox(id, slot, span) : (uint16_t)(slot * 61u);
}

struct Pool {
  uint32_t n_tiles = 0, n_buckets = 0, max_pieces = 0;
  uint64_t n_voxels = 0, records = 0;
  std::vector<uint32_t> tile, fill, nb;  // per id: tile (or TILE_INVALID) and fill; per tile: buckets
  unsigned long long* pool = nullptr;
  uint32_t *bucket_tile = nullptr, *bucket_fill = nullptr, *tile_nb = nullptr, *tile_start = nullptr,
           *cursor = nullptr, *dep_ctl = nullptr;
  uint2* order = nullptr;
  Piece* pieces = nullptr;
  double* jmean = nullptr;
  void release() {
    (void)hipFree(pool); (void)hipFree(bucket_tile); (void)hipFree(bucket_fill); (void)hipFree(tile_nb);
    (void)hipFree(tile_start); (void)hipFree(cursor); (void)hipFree(dep_ctl); (void)hipFree(order);
    (void)hipFree(pieces); (void)hipFree(jmean);
  }
};

// Upload the host description (tile, fill per id) and write the records.
static int upload(Pool& P) {
  P.n_buckets = (uint32_t)P.tile.size();
  P.nb.assign(P.n_tiles, 0);
  P.records = 0;
  for (uint32_t i = 0; i < P.n_buckets; ++i)
    if (P.tile[i] < P.n_tiles) { ++P.nb[P.tile[i]]; P.records += P.fill[i]; }
  const uint64_t cap = (uint64_t)P.n_buckets * BUCKET_RECORDS;
  P.max_pieces = (uint32_t)(cap / MIN_PIECE_RECORDS < REDUCE_PIECES + 1 ? cap / MIN_PIECE_RECORDS : REDUCE_PIECES + 1) + P.n_tiles + 1;
  const uint32_t nbk = P.n_buckets ? P.n_buckets : 1;
  CHECK(hipMalloc(&P.pool, (size_t)nbk * BUCKET_RECORDS * 8));
  CHECK(hipMalloc(&P.bucket_tile, (size_t)nbk * 4));
  CHECK(hipMalloc(&P.bucket_fill, (size_t)nbk * 4));
  CHECK(hipMalloc(&P.order, (size_t)nbk * sizeof(uint2)));
  CHECK(hipMalloc(&P.tile_nb, (size_t)P.n_tiles * 4));
  CHECK(hipMalloc(&P.tile_start, (size_t)P.n_tiles * 4));
  CHECK(hipMalloc(&P.cursor, (size_t)P.n_tiles * 4));
  CHECK(hipMalloc(&P.dep_ctl, 8 * 4));
  CHECK(hipMalloc(&P.pieces, (size_t)P.max_pieces * sizeof(Piece)));
  CHECK(hipMalloc(&P.jmean, (size_t)P.n_voxels * 8));
  if (P.n_buckets) {
    CHECK(hipMemcpy(P.bucket_tile, P.tile.data(), (size_t)P.n_buckets * 4, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(P.bucket_fill, P.fill.data(), (size_t)P.n_buckets * 4, hipMemcpyHostToDevice));
  }
  CHECK(hipMemcpy(P.tile_nb, P.nb.data(), (size_t)P.n_tiles * 4, hipMemcpyHostToDevice));
  // a stale list from an earlier fold: ids and fills that this fold must not use
  CHECK(hipMemset(P.order, 0x5a, (size_t)nbk * sizeof(uint2)));
  const uint32_t ctl[8] = {P.n_buckets, 0, 0, 0, 0, 0, 0, 0};  // [0]: ids handed out
  CHECK(hipMemcpy(P.dep_ctl, ctl, sizeof(ctl), hipMemcpyHostToDevice));
  CHECK(hipMemset(P.jmean, 0, (size_t)P.n_voxels * 8));
  if (P.n_buckets) {
    const uint64_t slots = (uint64_t)P.n_buckets * BUCKET_RECORDS;
    hipLaunchKernelGGL(fill_pool, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, 0, P.pool, P.bucket_tile,
                       P.bucket_fill, P.n_buckets, P.n_tiles, P.n_voxels);
    CHECK(hipGetLastError());
  }
  CHECK(hipDeviceSynchronize());
  return 0;
}

// The fold as enqueue_fold launches it (smcrt.hip), with bk_reduce on `blocks` blocks.
static int fold(const Pool& P, uint32_t blocks, bool lists) {
  if (lists) {
    hipLaunchKernelGGL(bk_scan, dim3(1), dim3(1024), 0, 0, P.tile_nb, P.n_tiles, P.tile_start, P.cursor, P.pieces,
                       P.dep_ctl);
    hipLaunchKernelGGL(bk_place, dim3(BIN_BLOCKS), dim3(BIN_THREADS), 0, 0, P.bucket_tile, P.bucket_fill, P.dep_ctl,
                       P.n_buckets, P.n_tiles, P.cursor, P.order);
  }
  hipLaunchKernelGGL(bk_reduce, dim3(blocks), dim3(RED_THREADS), 0, 0, P.pool, P.order, P.pieces, P.dep_ctl,
                     P.n_voxels, P.jmean, (unsigned long long*)nullptr);
  CHECK(hipGetLastError());
  return 0;
}

static int time_reduce(const Pool& P, uint32_t blocks, const char* name) {
  int dev = 0, cus = 0, khz = 0;
  CHECK(hipGetDevice(&dev));
  CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  CHECK(hipDeviceGetAttribute(&khz, hipDeviceAttributeClockRate, dev));
  hipEvent_t a, b;
  CHECK(hipEventCreate(&a)); CHECK(hipEventCreate(&b));
  if (fold(P, blocks, true)) return 1;  // warm-up, and the lists the timed runs read
  CHECK(hipDeviceSynchronize());
  float best = 1e30f;
  for (int rep = 0; rep < 3; ++rep) {
    CHECK(hipEventRecord(a));
    if (fold(P, blocks, false)) return 1;
    CHECK(hipEventRecord(b));
    CHECK(hipEventSynchronize(b));
    float ms = 0;
    CHECK(hipEventElapsedTime(&ms, a, b));
    if (ms < best) best = ms;
  }
  const int used = (int)blocks < cus ? (int)blocks : cus;  // one block per CU (128 KiB of LDS)
  printf("%-10s %5u blocks  %8.3f ms  %7.2f G records/s  %6.2f TB/s  %.3f records per CU-cycle (%d CUs, %d MHz)\n",
         name, blocks, best, P.records / best * 1e-6, P.records * 6.0 / best * 1e-9,
         P.records / (best * 1e-3) / used / (khz * 1e3), used, khz / 1000);
  CHECK(hipEventDestroy(a)); CHECK(hipEventDestroy(b));
  return 0;
}

static int bench(uint32_t tiles, uint32_t per_tile, uint32_t fill) {
  Pool P;
  P.n_tiles = tiles;
  P.n_voxels = (uint64_t)tiles * TILE_VOXELS;
  P.tile.resize((size_t)tiles * per_tile);
  P.fill.assign(P.tile.size(), fill);
  for (size_t i = 0; i < P.tile.size(); ++i) P.tile[i] = (uint32_t)(i % tiles);
  if (upload(P)) return 1;
  printf("fold_bench: %u tiles x %u buckets x %u records = %.1f M records (RED_GROUP %d)\n", tiles, per_tile, fill,
         P.records * 1e-6, RED_GROUP);
  const int rc = time_reduce(P, 1024, "whole chip") || time_reduce(P, 32, "32 blocks");
  P.release();
  return rc;
}

// One --check scene: per-tile bucket counts `nb`, fills from `fills` in turn, every seventh id retired.
static int check_scene(const char* name, const std::vector<uint32_t>& nb, const std::vector<uint32_t>& fills,
                       uint32_t last_span) {
  Pool P;
  P.n_tiles = (uint32_t)nb.size();
  P.n_voxels = (uint64_t)(P.n_tiles - 1) * TILE_VOXELS + last_span;
  std::vector<uint32_t> left(nb);
  uint32_t todo = 0;
  for (uint32_t c : nb) todo += c;
  uint32_t t = 0, k = 0;
  while (todo) {  // deal ids to the tiles that still want buckets, in turn
    if (P.tile.size() % 7 == 3) { P.tile.push_back(TILE_INVALID); P.fill.push_back(BUCKET_RECORDS); continue; }
    while (!left[t]) t = (t + 1) % P.n_tiles;
    P.tile.push_back(t);
    P.fill.push_back(fills[k++ % fills.size()]);
    --left[t]; --todo;
    t = (t + 1) % P.n_tiles;
  }
  if (upload(P)) return 1;
  std::vector<double> want(P.n_voxels, 0.0), got(P.n_voxels);
  for (uint32_t id = 0; id < P.n_buckets; ++id) {
    const uint32_t bt = P.tile[id];
    if (bt >= P.n_tiles) continue;
    const uint32_t span = bt + 1 == P.n_tiles ? last_span : TILE_VOXELS;
    for (uint32_t s = 0; s < P.fill[id]; ++s) want[(uint64_t)bt * TILE_VOXELS + rec_vox(id, s, span)] += (double)rec_val(id, s);
  }
  int bad = 0;
  for (uint32_t blocks : {1024u, 32u}) {
    CHECK(hipMemset(P.jmean, 0, (size_t)P.n_voxels * 8));
    if (fold(P, blocks, true)) return 1;
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(got.data(), P.jmean, (size_t)P.n_voxels * 8, hipMemcpyDeviceToHost));
    uint64_t diff = 0;
    for (uint64_t v = 0; v < P.n_voxels; ++v) diff += memcmp(&got[v], &want[v], 8) != 0;
    printf("check %-12s %4u blocks: %u ids, %llu records, %llu voxels differ%s\n", name, blocks, P.n_buckets,
           (unsigned long long)P.records, (unsigned long long)diff, diff ? "  FAILED" : "");
    bad |= diff != 0;
  }
  P.release();
  return bad;
}

static int check() {
  // tile t has t buckets (0..130), then two tiles that split into pieces (MIN_PIECE_BUCKETS per
  // piece), an empty tile and a last tile that n_voxels cuts
  std::vector<uint32_t> nb;
  for (uint32_t t = 0; t <= 130; ++t) nb.push_back(t);
  nb.push_back(MIN_PIECE_BUCKETS * 2 + 77);
  nb.push_back(MIN_PIECE_BUCKETS + 1);
  nb.push_back(0);
  nb.push_back(37);
  const std::vector<uint32_t> all = {1, 2, 3, 4, 5, 63, 64, 65, 255, 256};
  int bad = 0;
  for (uint32_t f : all) {
    char name[32];
    snprintf(name, sizeof name, "fill %u", f);
    bad |= check_scene(name, nb, {f}, 5000);
  }
  bad |= check_scene("mixed fills", nb, all, 5000);
  bad |= check_scene("one bucket", {0, 1}, {3}, 1);
  bad |= check_scene("no bucket", {0, 0, 0}, {1}, 100);
  printf(bad ? "fold_bench --check FAILED\n" : "fold_bench --check ok\n");
  return bad;
}

int main(int argc, char** argv) {
  uint32_t tiles = 128, per_tile = 32768, fill = BUCKET_RECORDS;
  bool chk = false;
  for (int i = 1; i < argc; ++i) {
    if (!strcmp(argv[i], "--check")) chk = true;
    else if (!strcmp(argv[i], "--tiles") && i + 1 < argc) tiles = (uint32_t)atoi(argv[++i]);
    else if (!strcmp(argv[i], "--buckets") && i + 1 < argc) per_tile = (uint32_t)atoi(argv[++i]);
    else if (!strcmp(argv[i], "--fill") && i + 1 < argc) fill = (uint32_t)atoi(argv[++i]);
    else { printf("usage: fold_bench [--check] [--tiles T] [--buckets B] [--fill F]\n"); return 2; }
  }
  if (!tiles || tiles > MAX_DIRECT_TILES || !fill || fill > BUCKET_RECORDS ||
      (uint64_t)tiles * per_tile >= BUCKET_ID_EXHAUSTED) {
    printf("fold_bench: need 1..%u tiles, fills 1..%u and fewer than %u buckets\n", MAX_DIRECT_TILES, BUCKET_RECORDS,
           BUCKET_ID_EXHAUSTED);
    return 2;
  }
  return chk ? check() : bench(tiles, per_tile, fill);
}
