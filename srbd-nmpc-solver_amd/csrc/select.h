// select.h -- a deterministic ascending stream compaction by one workgroup, shared by the
// kernels that list a subset of a batch: the unsolved QPs of the mixed-precision paths
// (rescue.hip) and the robots of an NMPC step that still iterate (srbd_linearize.hip).
#ifndef SRBD_SELECT_H_
#define SRBD_SELECT_H_
#include <hip/hip_runtime.h>

namespace srbd {
namespace {

constexpr int kSelThreads = 1024;

// One workgroup of kSelThreads (wave64) walks positions 0 .. n-1 in 1024-entry tiles: per wave
// a ballot of the flags and its prefix popcount, per tile a 16-entry prefix over the waves.
// pick(i, &value) is called once per position, by the thread that owns it; where it returns
// true, `value` is appended to idx[].  The kept values stand in position order (a stable
// compaction: deterministic, and ascending where the values ascend with the position);
// *count receives how many.  idx may not alias what pick reads at other positions.
template <class Pick>
__device__ __forceinline__ void select_in_order(int n, int* __restrict__ idx, int* __restrict__ count,
                                                Pick&& pick) {
  __shared__ int wave_tot[kSelThreads / 64];
  __shared__ int wave_off[kSelThreads / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int base_out = 0;
  for (int base = 0; base < n; base += kSelThreads) {
    const int i = base + (int)threadIdx.x;
    int value = i;
    const bool flag = i < n && pick(i, value);
    const unsigned long long m = __ballot(flag);
    const int before = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wave_tot[wave] = __popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
      int run = 0;
      for (int w = 0; w < kSelThreads / 64; ++w) {
        wave_off[w] = run;
        run += wave_tot[w];
      }
      wave_tot[0] = run;  // tile total (wave_tot is re-written next tile after the barrier)
    }
    __syncthreads();
    if (flag) idx[base_out + wave_off[wave] + before] = value;
    base_out += wave_tot[0];
    __syncthreads();
  }
  if (threadIdx.x == 0) *count = base_out;
}

}  // namespace
}  // namespace srbd
#endif  // SRBD_SELECT_H_
