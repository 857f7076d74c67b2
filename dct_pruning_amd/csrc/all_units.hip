// all_units.hip - the codelet, split, fused, two-roles and pipelined families and the C ABI (api.hip, host code) in ONE translation unit; the other units are compiled beside it:
// `make single` and the stamp diagnostics (-DDCTS_FUSED_STAMPS: g_fused_stamps is one __device__ symbol written by three families and read by api.hip).
#include "codelet.hip"
#include "split.hip"
#include "split_more.hip"
#include "fused.hip"
#include "fused2.hip"
#include "pipe.hip"
#include "api.hip"
