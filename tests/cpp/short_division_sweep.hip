// Stand-alone host check of the three-operation division by a known focal length (devmath.hpp: div_short,
// short_division_proven).  Host code only; built with hipcc because devmath.hpp includes the HIP headers:
//   hipcc -O2 -std=c++17 -ffp-contract=off -fno-fast-math -Ialign3d_amd/csrc -o short_division_sweep tests/cpp/short_division_sweep.hip
//   ./short_division_sweep <random focal lengths> [focal length ...]
// 1. For every focal length given (the sample camera's by default): q = a y, r = fma(-f, q, a), q' = fma(r, y, q) with
//    y = RN(1 / f) against a / f over all 2^23 mantissas of a, written here independently of the library's sweep, and
//    the library's verdict must agree; then 2^20 random numerators of either sign over the whole admitted range
//    1e-20 < |a| < 1e9 (the sweep covers one binade and relies on exact scaling for the rest) and +0.
// 2. The same full sweep for N random focal lengths (log-uniform in 1e-2 .. 1e5, either sign): how many pass is printed,
//    a finding and not a gate, with the first few that fail; the library's verdict must agree for each.
// Exit status 0 when every sample focal length passes and every verdict agrees.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "devmath.hpp"

static float short_div(float a, float f, float y) {
  const float q = a * y;
  const float r = std::fmaf(-f, q, a);
  return std::fmaf(r, y, q);
}
static bool same_bits(float a, float b) { return memcmp(&a, &b, 4) == 0; }

static uint32_t sweep_mismatches(float f) {
  const float y = 1.0f / f;
  uint32_t bad = 0;
  for (uint32_t m = 0; m < (1u << 23); ++m) {
    const uint32_t bits = 0x3f800000u | m;
    float a;
    memcpy(&a, &bits, 4);
    bad += !same_bits(short_div(a, f, y), a / f);
  }
  return bad;
}

int main(int argc, char** argv) {
  const int n_random = argc > 1 ? atoi(argv[1]) : 100;
  std::vector<float> samples;
  for (int i = 2; i < argc; ++i) samples.push_back((float)atof(argv[i]));
  if (samples.empty()) samples = {544.4732666015625f, 544.4732666015625f * 24.0f / 640.0f, 544.4732666015625f * 64.0f / 640.0f, 525.0f};
  int failures = 0;
  std::mt19937_64 rng(12345);
  for (float f : samples) {
    const uint32_t bad = sweep_mismatches(f);
    const bool verdict = a3d::short_division_proven(f);
    uint32_t bad_range = 0;
    const float y = 1.0f / f;
    std::uniform_real_distribution<double> ex(-20.0, 9.0), man(1.0, 10.0);
    for (int k = 0; k < (1 << 20); ++k) {
      float a = (float)(man(rng) * std::pow(10.0, ex(rng) - 1.0));
      if (!(std::fabs(a) > 1e-20f && std::fabs(a) < 1e9f)) continue;
      if (k & 1) a = -a;
      bad_range += !same_bits(short_div(a, f, y), a / f);
    }
    const bool zero_ok = !(f > 0.0f) || same_bits(short_div(0.0f, f, y), 0.0f);
    printf("sample f = %.9g: %u of 8388608 mantissas differ, %u random numerators over the range differ, +0 %s, library verdict %d\n",
           f, bad, bad_range, zero_ok ? "ok" : "WRONG", (int)verdict);
    if (bad || bad_range || !zero_ok || !verdict) ++failures;
  }
  int passed = 0, shown = 0, disagree = 0;
  std::uniform_real_distribution<double> lf(-2.0, 5.0);
  for (int k = 0; k < n_random; ++k) {
    float f = (float)std::pow(10.0, lf(rng));
    if (k & 1) f = -f;
    const uint32_t bad = sweep_mismatches(f);
    if (a3d::short_division_proven(f) != (bad == 0)) ++disagree;
    if (bad == 0) {
      ++passed;
    } else if (shown < 8) {
      printf("fails: f = %.9g (0x%08x), %u mantissas\n", f, [&] { uint32_t b; memcpy(&b, &f, 4); return b; }(), bad);
      ++shown;
    }
  }
  printf("random focal lengths: %d of %d pass, %d verdicts disagree\n", passed, n_random, disagree);
  return (failures || disagree) ? 1 : 0;
}
