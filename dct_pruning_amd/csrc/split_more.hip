// split_more.hip - the two-launch split family for the 8 * M edges of round 3 (DCTS_SPLIT_TABLE_MORE_B): a unit of its
// own so that these instantiations compile in parallel with those of split.hip.
#include "../../include/dctscore.h"
#include "codelet_sizes.h"
#include "split_kernels.hpp"

using namespace dctsi;

#ifdef DCTS_SPLIT_TABLE_MORE_B
namespace dctsi {

int dispatch_split_more(int N, const MapGeom& g, float* out, void* workspace, hipStream_t st) {
#define DCTS_CASE(N_, M_, L_) \
  case N_:                    \
    return launch_split<M_, L_>(g, out, workspace, st);
  switch (N) {
    DCTS_SPLIT_TABLE_MORE_B(DCTS_CASE)
    default:
      return DCTS_E_UNSUPPORTED;
  }
#undef DCTS_CASE
}

}  // namespace dctsi
#endif
