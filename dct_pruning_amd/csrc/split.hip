// split.hip - the two-launch split family: workspace layout, and the dispatcher for every edge of DCTS_SPLIT_TABLE
// except the 8 * M edges of round 3 (split_more.hip).
#include <stdlib.h>

#include "../../include/dctscore.h"
#include "codelet_sizes.h"
#include "split_kernels.hpp"

using namespace dctsi;

namespace {

// intermediate tile buffer per launch pair; DCTS_SPLIT_CHUNK_MB overrides (tuning knob)
size_t split_chunk_bytes() {
  static const size_t v = [] {
    const char* e = getenv("DCTS_SPLIT_CHUNK_MB");
    long mb = e ? atol(e) : 0;
    if (mb < 1 || mb > 4096) mb = 256;
    return (size_t)mb << 20;
  }();
  return v;
}

}  // namespace

namespace dctsi {

int split_partials_per_map(int N) {
#define DCTS_CASE(N_, M_, L_) \
  if (N == N_) return SplitCfg<M_, L_>::STRIPS * SplitCfg<M_, L_>::ROLES;
  DCTS_SPLIT_TABLE(DCTS_CASE)
#undef DCTS_CASE
  return 0;
}

SplitWs split_ws(long long nmaps, int N) {
  SplitWs w;
  const size_t map_bytes = (size_t)N * N * 4;
  long long chunk = (long long)(split_chunk_bytes() / map_bytes);
  if (chunk < 1) chunk = 1;
  if (chunk > nmaps) chunk = nmaps;
  w.chunk_maps = chunk;
  w.off_t = 0;
  w.off_part = align_up((size_t)chunk * map_bytes, 256);
  w.total = align_up(w.off_part + (size_t)chunk * split_partials_per_map(N) * 4, 256);
  return w;
}

int dispatch_split(int N, const MapGeom& g, float* out, void* workspace, hipStream_t st) {
#define DCTS_CASE(N_, M_, L_) \
  case N_:                    \
    return launch_split<M_, L_>(g, out, workspace, st);
  switch (N) {
#ifdef DCTS_SPLIT_TABLE_MORE_A
    DCTS_SPLIT_TABLE_BASE(DCTS_CASE)
    DCTS_SPLIT_TABLE_MORE_A(DCTS_CASE)
    default:
      return dispatch_split_more(N, g, out, workspace, st);
#else
    DCTS_SPLIT_TABLE(DCTS_CASE)
    default:
      return DCTS_E_UNSUPPORTED;
#endif
  }
#undef DCTS_CASE
}

}  // namespace dctsi
