// The sliding-window plan, the reflection and the ramp weights of include/vit_unet_amd.h ("Whole-image restoration"), shared by
// csrc/vu_tile.hip (restoration) and csrc/vu_segtile.hip (segmentation): one definition, so that a logit blended by the
// segmentation kernel is bit for bit what vu_tile_blend gives the same window outputs.
//
// Plan, per axis of length L (stride S = T - overlap, 0 <= overlap <= T/2):
//   L <= T: one window at 0; the T - L missing rows / columns are reflected without repeating the edge, and only the
//           first L rows / columns of that window's output are used;
//   L >  T: n = ceil((L - T) / S) + 1 windows at min(i S, L - T): the last window is shifted inwards, not padded.
// Weight of window pixel i along one axis: min(i + 1, T - i, overlap + 1) / (overlap + 1), positive everywhere.
#pragma once
#include "vu_common.h"

namespace {

struct tile_axis {
  int L, T, S, ov, n;
};

inline int axis_count(int L, int T, int S) { return L <= T ? 1 : (int)vu_cdiv64((long long)L - T, S) + 1; }

inline tile_axis make_axis(int L, int T, int overlap) {
  tile_axis a;
  a.L = L; a.T = T; a.ov = overlap; a.S = T - overlap;
  a.n = axis_count(L, T, a.S);
  return a;
}

__host__ __device__ __forceinline__ int axis_origin(const tile_axis& a, int i) {
  const int r = i * a.S, last = a.L - a.T;
  return a.L <= a.T ? 0 : (r < last ? r : last);
}

// the first window (in plan order) that covers pixel p; the ones after it cover p while their origin is <= p
__device__ __forceinline__ int axis_first(const tile_axis& a, int p) {
  if (a.L <= a.T || p < a.T) return 0;
  return min((p - a.T) / a.S + 1, a.n - 1);
}

// source index of window position k = origin + i: the pixel itself, or (L < T only) its reflection without the edge
__device__ __forceinline__ int axis_src(const tile_axis& a, int k) {
  if (k < a.L) return k;
  if (a.L == 1) return 0;
  const int m = 2 * (a.L - 1);
  k %= m;
  return k < a.L ? k : m - k;
}

__device__ __forceinline__ float axis_weight(const tile_axis& a, int i) {
  return __fdiv_rn((float)min(min(i + 1, a.T - i), a.ov + 1), (float)(a.ov + 1));
}

int check_plan(const char* who, int H, int W, int T, int overlap) {
  VU_REQUIRE(T > 0, "%s: the window size must be positive (got %d)", who, T);
  VU_REQUIRE(H > 0 && W > 0, "%s: empty image (%d x %d)", who, H, W);
  VU_REQUIRE(overlap >= 0 && overlap <= T / 2, "%s: overlap must be in 0 .. T/2 = %d (got %d)", who, T / 2, overlap);
  return VU_OK;
}

}  // namespace
