// The fixed inputs of the stand-alone programs of tests/psis_host ... tests/loo_ap_host (-DPPCX_HOST_MAIN; built and run under
// the host sanitizers by `python -m tests.host_build --sanitize`): columns at the draw counts where indexing can go wrong, clean,
// with one NaN and with one -Inf. No files, no arguments.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <vector>

namespace host_main {

// one draw; either side of the PSIS minimum tail (M = 4 at 20 draws, 5 at 21); a few hundred
const long kDraws[] = {1, 20, 21, 300};
enum Kind { CLEAN, WITH_NAN, WITH_MINUS_INF };
const Kind kKinds[] = {CLEAN, WITH_NAN, WITH_MINUS_INF};
const char* const kKindNames[] = {"clean", "nan", "-inf"};

// n values around `centre` that neither repeat nor tie; the middle one replaced as `kind` says
inline std::vector<double> column(long n, Kind kind, double centre = -3.0, double phase = 0.0) {
  std::vector<double> v((size_t)n);
  for (long i = 0; i < n; ++i) v[i] = centre + 0.8 * sin(1.7 * (double)i + phase) + 0.3 * cos(0.31 * (double)i * (double)i);
  if (kind == WITH_NAN) v[n / 2] = NAN;
  if (kind == WITH_MINUS_INF) v[n / 2] = -INFINITY;
  return v;
}
// counts drawn around 100, one per draw
inline std::vector<int32_t> counts(long n) {
  std::vector<int32_t> x((size_t)n);
  for (long i = 0; i < n; ++i) x[i] = 100 + (int32_t)(40.0 * sin(0.9 * (double)i));
  return x;
}
inline bool all_nan(const double* out, int fields) {
  for (int f = 0; f < fields; ++f) if (!isnan(out[f])) return false;
  return true;
}
inline int impossible(const char* what) { printf("impossible result: %s\n", what); return 1; }

}  // namespace host_main
