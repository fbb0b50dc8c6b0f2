// The host front of the batched resident-cloud calls (cloud_batch.hpp, voxel_grid.hpp, cell_sort.hpp) on its own: a
// plain C++17 program with no device and no library, built with AddressSanitizer and UBSan by
// tests/test_cloud_batch_host_cpu.py.  Every address is made up and none is dereferenced.  Exit status 0 = all held.
#include <cinttypes>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "cell_sort.hpp"
#include "cloud_batch.hpp"

static char g_error[512];
namespace a3d {
void set_error(const char* fmt, ...) {  // (the library's own is in context.hip)
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_error, sizeof g_error, fmt, ap);
  va_end(ap);
}
}  // namespace a3d
using namespace a3d;

#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      exit(1);                                                        \
    }                                                                 \
  } while (0)

template <class T>
static T* at(uintptr_t address) {
  return reinterpret_cast<T*>(address);
}

struct Span {
  uintptr_t begin;
  uint64_t bytes;
  bool output;
};

static bool overlap_of(const std::vector<Span>& spans) {
  RangeRecorder r;
  for (const Span& s : spans) s.output ? r.out(at<char>(s.begin), s.bytes) : r.in(at<char>(s.begin), s.bytes);
  return r.overlap();
}

// The same answer for every insertion order of the spans.
static bool overlap_any_order(std::vector<Span> spans) {
  std::vector<size_t> order(spans.size());
  for (size_t i = 0; i < order.size(); ++i) order[i] = i;
  const bool first = overlap_of(spans);
  do {
    std::vector<Span> permuted;
    for (size_t i : order) permuted.push_back(spans[i]);
    CHECK(overlap_of(permuted) == first);
  } while (std::next_permutation(order.begin(), order.end()));
  return first;
}

static void test_recorder() {
  RangeRecorder r;
  r.in(nullptr, 48), r.out(nullptr, 48), r.in(at<char>(0x1000), 0), r.out(at<char>(0x1000), 0);
  CHECK(r.size() == 0 && !r.overlap());
  r.in(at<char>(0x1000), 48), r.out(at<char>(0x2000), 48);
  CHECK(r.size() == 2 && !r.overlap());
  const bool IN = false, OUT = true;
  CHECK(!overlap_any_order({{0x1000, 48, IN}, {0x1000, 48, IN}, {0x1010, 100, IN}}));  // inputs over inputs
  CHECK(overlap_any_order({{0x1000, 48, IN}, {0x1000, 48, OUT}}));                     // exactly in place
  CHECK(overlap_any_order({{0x1000, 48, IN}, {0x102F, 48, OUT}}));                     // the output's first byte on the input's last
  CHECK(overlap_any_order({{0x1000, 48, OUT}, {0x102F, 48, IN}}));                     // the input's first byte on the output's last
  CHECK(overlap_any_order({{0x1000, 48, OUT}, {0x102F, 1, OUT}}));                     // two outputs, one byte shared
  CHECK(!overlap_any_order({{0x1000, 48, IN}, {0x1030, 48, OUT}}));                    // they touch
  CHECK(!overlap_any_order({{0x1000, 48, OUT}, {0x1030, 48, IN}}));
  CHECK(!overlap_any_order({{0x1000, 48, OUT}, {0x1030, 48, OUT}, {0x1060, 4, OUT}}));
  CHECK(overlap_any_order({{0x1000, 400, OUT}, {0x1100, 4, IN}}));                     // an input inside an output
  CHECK(overlap_any_order({{0x1000, 400, IN}, {0x1100, 4, OUT}}));                     // an output inside an input
  // a long input hides nothing: the output behind a short input still meets it
  CHECK(overlap_any_order({{0x1000, 400, IN}, {0x1010, 4, IN}, {0x1100, 4, OUT}}));
  CHECK(overlap_any_order({{0x1000, 400, OUT}, {0x1010, 4, OUT}, {0x1100, 4, IN}, {0x3000, 8, IN}}));
  CHECK(!overlap_any_order({{0x1000, 16, IN}, {0x1008, 16, IN}, {0x1018, 8, OUT}, {0x1020, 8, IN}}));
}

// A job with the field names the compacting calls share (SelectJob, VoxelJob and MeanJob each have these and their own).
struct DummyJob {
  const float* points;
  const float* normals;
  float* out_points;
  float* out_normals;
  uint32_t* out_index;
  unsigned long long capacity;
  uint32_t len, first_tile, chunks_per_tile, pad;
  const uint8_t* colors;
  uint8_t* out_colors;
};

constexpr uint32_t CHUNK = 1024, MAX_TILES = 4096;

struct Clouds {  // two clouds of 4 points, every array of each at its own made-up address
  a3d_point_cloud_view views[2] = {{at<float>(0x10000), at<float>(0x20000), 4}, {at<float>(0x30000), at<float>(0x38000), 4}};
  const uint8_t* colors[2] = {at<uint8_t>(0x40000), at<uint8_t>(0x48000)};
  float* out_points[2] = {at<float>(0x50000), at<float>(0x58000)};
  float* out_normals[2] = {at<float>(0x60000), at<float>(0x68000)};
  uint8_t* out_colors[2] = {at<uint8_t>(0x70000), at<uint8_t>(0x78000)};
  uint32_t* out_index[2] = {at<uint32_t>(0x80000), at<uint32_t>(0x88000)};
  uint64_t capacities[2] = {4, 4};
  CompactArgs args() const { return CompactArgs{views, colors, out_points, out_normals, out_colors, out_index, capacities}; }
};

static a3d_status front(const Clouds& c, uint64_t i, bool others, RangeRecorder* ranges, DummyJob* j, uint64_t* tiles) {
  g_error[0] = 0;
  return compact_front("the_entry_point", c.args(), i, others, "null points or output pointer", CHUNK, MAX_TILES, tiles,
                       ranges, j);
}

static void test_compact_front() {
  uint64_t tiles = 0;
  {  // a good cloud: every field, its tiles, three inputs and four outputs
    Clouds c;
    RangeRecorder ranges;
    DummyJob j{};
    CHECK(front(c, 1, true, &ranges, &j, &tiles) == A3D_OK && g_error[0] == 0);
    CHECK(j.points == c.views[1].points && j.normals == c.views[1].normals && j.colors == c.colors[1]);
    CHECK(j.out_points == c.out_points[1] && j.out_normals == c.out_normals[1] && j.out_colors == c.out_colors[1]);
    CHECK(j.out_index == c.out_index[1] && j.capacity == 4 && j.len == 4 && j.first_tile == 0 && j.chunks_per_tile == 1);
    CHECK(tiles == 1 && ranges.size() == 7 && !ranges.overlap());
  }
  {  // no optional array at all: the job's optional fields are null, two ranges
    Clouds c;
    CompactArgs a = c.args();
    a.colors = nullptr, a.out_normals = nullptr, a.out_colors = nullptr, a.out_index = nullptr;
    RangeRecorder ranges;
    DummyJob j{};
    CHECK(compact_front("e", a, 0, true, "nulls", CHUNK, MAX_TILES, &tiles, &ranges, &j) == A3D_OK);
    CHECK(!j.normals && !j.colors && !j.out_normals && !j.out_colors && !j.out_index && ranges.size() == 2);
    CHECK(j.first_tile == 1 && tiles == 2);
  }
  // the order of the refusals: nulls, then normals, then colours, then the tile plan; nothing is recorded by a refusal
  for (int what = 0; what < 3; ++what) {
    Clouds c;
    c.views[0].normals = nullptr, c.colors[0] = nullptr, c.views[0].len = 0xFFFFFFFFull;  // three later refusals wait
    if (what == 0) c.views[0].points = nullptr;
    if (what == 1) c.out_points[0] = nullptr;
    RangeRecorder ranges;
    DummyJob j{};
    uint64_t t = 0;
    CHECK(front(c, 0, what != 2, &ranges, &j, &t) == A3D_INVALID_PARAMETER);
    CHECK(!strcmp(g_error, "the_entry_point: null points or output pointer") && ranges.size() == 0 && t == 0);
  }
  {
    Clouds c;
    c.views[0].normals = nullptr, c.colors[0] = nullptr, c.views[0].len = 0xFFFFFFFFull;
    RangeRecorder ranges;
    DummyJob j{};
    uint64_t t = 0;
    CHECK(front(c, 0, true, &ranges, &j, &t) == A3D_MISSING_FIELD && !strcmp(g_error, "the_entry_point: cloud has no normals"));
    c.views[0].normals = at<float>(0x20000);
    CHECK(front(c, 0, true, &ranges, &j, &t) == A3D_MISSING_FIELD && !strcmp(g_error, "the_entry_point: cloud has no colours"));
    CompactArgs a = c.args();
    a.colors = nullptr;  // no colours array at all, and a colours output
    CHECK(compact_front("e", a, 0, true, "nulls", CHUNK, MAX_TILES, &t, &ranges, &j) == A3D_MISSING_FIELD);
    c.colors[0] = at<uint8_t>(0x40000);
    CHECK(front(c, 0, true, &ranges, &j, &t) == A3D_INVALID_PARAMETER);
    CHECK(!strcmp(g_error, "the_entry_point: a cloud within one tile of 2^32 points") && ranges.size() == 0);
    // a missing field that nobody asks for is no refusal
    Clouds d;
    d.views[0].normals = nullptr, d.colors[0] = nullptr, d.out_normals[0] = nullptr, d.out_colors[0] = nullptr;
    CHECK(front(d, 0, true, &ranges, &j, &t) == A3D_OK && !j.normals && !j.colors && ranges.size() == 3);
  }
  // the outputs count for their first min(len, capacity) elements
  for (uint64_t capacity : {0ull, 2ull, 4ull, 9ull}) {
    Clouds c;
    c.capacities[0] = capacity;
    const uint64_t kept = std::min<uint64_t>(4, capacity);
    RangeRecorder ranges;
    DummyJob j{};
    uint64_t t = 0;
    CHECK(front(c, 0, true, &ranges, &j, &t) == A3D_OK && j.capacity == capacity);
    CHECK(ranges.size() == (kept ? 7u : 3u));
    // an input right behind what may be written touches it; one byte earlier it is written over
    struct {
      uintptr_t base;
      uint64_t element;
    } outs[] = {{0x50000, 12}, {0x60000, 12}, {0x70000, 3}, {0x80000, 4}};
    for (const auto& o : outs) {
      RangeRecorder touching = ranges, inside = ranges;
      touching.in(at<char>(o.base + kept * o.element), 64);
      CHECK(!touching.overlap());
      if (kept) {
        inside.in(at<char>(o.base + kept * o.element - 1), 64);
        CHECK(inside.overlap());
      }
    }
    RangeRecorder in_place = ranges;  // an output on its own input
    in_place.out(at<char>(0x10000), 1);
    CHECK(in_place.overlap());
  }
  // the tiles are plan_tiles' own, job after job
  uint64_t mine = 0, direct = 0;
  for (uint64_t len : {(uint64_t)1, (uint64_t)CHUNK - 1, (uint64_t)CHUNK, (uint64_t)CHUNK + 1, (uint64_t)MAX_TILES * CHUNK + 1,
                       (uint64_t)3 * MAX_TILES * CHUNK}) {
    Clouds c;
    c.views[0].len = len;
    RangeRecorder ranges;
    DummyJob j{};
    uint32_t first_tile = 0, chunks_per_tile = 0;
    CHECK(front(c, 0, true, &ranges, &j, &mine) == A3D_OK);
    CHECK(plan_tiles(len, CHUNK, MAX_TILES, &direct, &first_tile, &chunks_per_tile) == A3D_OK);
    CHECK(j.len == len && j.first_tile == first_tile && j.chunks_per_tile == chunks_per_tile && mine == direct);
    const uint64_t chunks = (len + CHUNK - 1) / CHUNK, job_tiles = mine - j.first_tile;
    CHECK(job_tiles <= MAX_TILES && job_tiles * j.chunks_per_tile >= chunks && (job_tiles - 1) * j.chunks_per_tile < chunks);
  }
  CHECK(mine == 1 + 1 + 1 + 2 + 2049 + 4096);
}

static void test_compact_finish() {
  std::vector<DummyJob> jobs(2);
  jobs[0].capacity = 5, jobs[1].capacity = 7;
  const std::vector<uint64_t> cloud_of_job{0, 2};  // cloud 1 was empty
  unsigned long long words[] = {5, 7, 11, 13};
  uint64_t lens[3] = {77, 77, 77}, dropped[3] = {77, 77, 77};
  zero_results(lens, 3), zero_results(nullptr, 3);
  CHECK(lens[0] == 0 && lens[1] == 0 && lens[2] == 0);
  CHECK(compact_finish("e", "rows", jobs, cloud_of_job, words, lens, dropped) == A3D_OK);
  CHECK(lens[0] == 5 && lens[1] == 0 && lens[2] == 7 && dropped[0] == 11 && dropped[1] == 77 && dropped[2] == 13);
  words[1] = 8;  // one over its capacity: the counts still go out, then the refusal
  CHECK(compact_finish("the_entry_point", "kept rows", jobs, cloud_of_job, words, lens, nullptr) == A3D_INVALID_PARAMETER);
  CHECK(lens[2] == 8 && !strcmp(g_error, "the_entry_point: a capacity is smaller than its cloud's kept rows (nothing was written)"));
  uint64_t stats[12];
  zero_results(stats, 3, 4);
  const unsigned long long runs[] = {1, 2, 3, 4, 5, 6, 7, 8};
  scatter_words(runs, cloud_of_job, stats, 4);
  const uint64_t want[12] = {1, 2, 3, 4, 0, 0, 0, 0, 5, 6, 7, 8};
  CHECK(!memcmp(stats, want, sizeof want));
}

struct SortJob {  // what cell_sort_plan fills (KnnJob, NormalsJob)
  const float* points;
  VoxelSlot* table;
  CellRecord* sorted;
  unsigned long long slot_mask;
  uint32_t len, first_tile, chunks_per_tile, n_tiles;
  unsigned long long* flags;  // (a part of the caller's own)
};

static void test_tail_parts() {
  // three jobs, two parts, as the voxel downsample carves them: ballot words (padded per job) | hash tables (not padded)
  const uint64_t lens[3] = {1, 4097, 70000};
  struct {
    unsigned long long* flags;
    VoxelSlot* table;
  } jobs[3];
  TailPart flags, tables;
  size_t flag_bytes = 0, table_bytes = 0, flag_at[3], table_at[3];
  for (int q = 0; q < 3; ++q) {
    const uint64_t slots = table_slots(lens[q]);
    flags.take(&jobs[q].flags, pad256((lens[q] + 63) / 64 * 8)), tables.take(&jobs[q].table, slots * sizeof(VoxelSlot));
    flag_at[q] = flag_bytes, table_at[q] = table_bytes;  // the hand computation of the entry points before this helper
    flag_bytes += pad256((lens[q] + 63) / 64 * 8), table_bytes += slots * sizeof(VoxelSlot);
    CHECK((size_t)jobs[q].flags == flag_at[q] && (size_t)jobs[q].table == table_at[q]);
  }
  CHECK(flags.bytes == flag_bytes && tables.bytes == table_bytes);
  CHECK(flag_at[1] == 256 && flag_at[2] == 256 + 768 && flag_bytes == 256 + 768 + 8960);
  CHECK(table_at[1] == 2 * 16 && table_at[2] == (2 + 16384) * 16 && table_bytes == (2 + 16384 + 262144) * 16);
  char* tail = at<char>(0x7f0000000100);
  place_parts(tail, {&flags, &tables});
  CHECK(flags.base == tail && tables.base == tail + flag_bytes);
  for (int q = 0; q < 3; ++q) {
    flags.rebase(&jobs[q].flags), tables.rebase(&jobs[q].table);
    CHECK((char*)jobs[q].flags == tail + flag_at[q] && (char*)jobs[q].table == tail + flag_bytes + table_at[q]);
    CHECK((uintptr_t)jobs[q].flags % 256 == 0);
  }
  // the counting sort's plan: hash tables | (a part of the caller) | records, as the clustering lays them out
  CellSortPlan plan;
  TailPart between;
  SortJob sort[3] = {};
  size_t sorted_at[3], sorted_bytes = 0;
  uint64_t tiles = 0;
  for (int q = 0; q < 3; ++q) {
    CHECK(cell_sort_plan(&plan, "e", lens[q], &sort[q]) == A3D_OK);
    between.take(&sort[q].flags, pad256(lens[q] * 4));
    uint32_t first_tile, chunks_per_tile;
    CHECK(plan_tiles(lens[q], CELL_CHUNK, CELL_MAX_TILES, &tiles, &first_tile, &chunks_per_tile) == A3D_OK);
    CHECK(sort[q].len == lens[q] && sort[q].first_tile == first_tile && sort[q].chunks_per_tile == chunks_per_tile);
    CHECK(sort[q].n_tiles == tiles - first_tile && plan.tiles == tiles && sort[q].slot_mask == table_slots(lens[q]) - 1);
    sorted_at[q] = sorted_bytes, sorted_bytes += pad256(lens[q] * sizeof(CellRecord));
    CHECK((size_t)sort[q].table == table_at[q] && (size_t)sort[q].sorted == sorted_at[q]);
  }
  CHECK(plan.tables.bytes == table_bytes && plan.sorted.bytes == sorted_bytes && sorted_at[1] == 256);
  place_parts(tail, {&plan.tables, &between, &plan.sorted});
  for (int q = 0; q < 3; ++q) {
    cell_sort_rebase(plan, &sort[q]);
    CHECK((char*)sort[q].table == tail + table_at[q]);
    CHECK((char*)sort[q].sorted == tail + table_bytes + between.bytes + sorted_at[q]);
  }
  SortJob far{};
  CHECK(cell_sort_plan(&plan, "the_entry_point", 0xFFFFFFFFull, &far) == A3D_INVALID_PARAMETER);
  CHECK(!strcmp(g_error, "the_entry_point: a cloud within one tile of 2^32 points"));
}

static void test_table_slots() {
  CHECK(table_slots(0) == 2 && table_slots(1) == 2 && table_slots(2) == 4 && table_slots(3) == 8);
  for (int k = 2; k <= 32; ++k)
    for (uint64_t len : {(1ull << k) - 1, 1ull << k, (1ull << k) + 1}) {
      const uint64_t slots = table_slots(len);
      CHECK((slots & (slots - 1)) == 0 && slots >= 2 * len && slots < 4 * len);
      const uint64_t floored = table_slots(len, 64);
      CHECK(floored == std::max<uint64_t>(slots, 64));
    }
  CHECK(table_slots(0, 64) == 64 && table_slots(32, 64) == 64 && table_slots(33, 64) == 128);
}

static void test_argument_checks() {
  VoxelGrid g{};
  const float origin[3] = {1.f, -2.f, 3.f}, bad[3] = {0.f, INFINITY, 0.f};
  CHECK(voxel_grid_from("e", 0.5f, nullptr, &g) == A3D_OK && g.v == 0.5f && g.ox == 0.f && g.oy == 0.f && g.oz == 0.f);
  CHECK(voxel_grid_from("e", 0.5f, origin, &g) == A3D_OK && g.ox == 1.f && g.oy == -2.f && g.oz == 3.f);
  for (float v : {0.f, -0.f, -1.f, NAN, INFINITY, -INFINITY}) {
    CHECK(voxel_grid_from("the_entry_point", v, bad, &g) == A3D_INVALID_PARAMETER);  // the size is looked at first
    CHECK(!strcmp(g_error, "the_entry_point: the voxel size must be finite and positive"));
  }
  CHECK(voxel_grid_from("the_entry_point", 1.f, bad, &g) == A3D_INVALID_PARAMETER);
  CHECK(!strcmp(g_error, "the_entry_point: the origin must be finite"));
  float r2 = 0.f, s = 0.f;
  CHECK(radius_grid_from("e", 0.25f, &g, &r2, &s) == A3D_OK && g.v == 0.25f && g.ox == 0.f && r2 == 0.0625f && s == 131072.f);
  CHECK(radius_grid_from("e", 0.25f, &g, &r2, nullptr) == A3D_OK);
  for (float r : {0.f, -1.f, NAN, INFINITY}) {
    CHECK(radius_grid_from("the_entry_point", r, &g, &r2, &s) == A3D_INVALID_PARAMETER);
    CHECK(!strcmp(g_error, "the_entry_point: the radius must be finite and positive"));
  }
  for (float r : {1e-23f, 1e-36f}) {  // r * r is 0 in f32 / 32768 / r is not finite
    CHECK(radius_grid_from("the_entry_point", r, &g, &r2, &s) == A3D_INVALID_PARAMETER);
    CHECK(!strcmp(g_error, "the_entry_point: a radius whose square is 0 in f32 (below about 1e-19)"));
  }
}

int main() {
  test_recorder();
  test_compact_front();
  test_compact_finish();
  test_tail_parts();
  test_table_slots();
  test_argument_checks();
  printf("cloud_batch_host_test: ok\n");
  return 0;
}
