// Whole-image restoration: sliding-window inference around the model's own resolution.  An H x W image is covered by
// T x T windows (T = im_size) that overlap by `overlap` pixels; vu_tile_gather_* cut the windows of the plan into the
// (n,C,T,T) batch the eval forward takes, vu_tile_blend puts the window outputs back together with a separable ramp
// weight, normalised per pixel.  The inverse of the device input pipeline (csrc/vu_data.hip), which only resizes.
//
// Plan, per axis of length L (stride S = T - overlap, 0 <= overlap <= T/2):
//   L <= T: one window at 0; the T - L missing rows / columns are reflected without repeating the edge, and only the
//           first L rows / columns of that window's output are used;
//   L >  T: n = ceil((L - T) / S) + 1 windows at min(i S, L - T): the last window is shifted inwards, not padded.
// The 2-D plan is the outer product, row-major (ty outer, tx inner).  A pixel is covered by at most 3 windows per axis.
// Weight of window pixel i along one axis: min(i + 1, T - i, overlap + 1) / (overlap + 1), positive everywhere.
//
// Both kernels are pure streaming: no reuse beyond the overlap (served by L2), one thread = 4 consecutive pixels of a
// row, 16-byte accesses on the float side wherever the addresses allow it (window rows are 16-byte aligned when T % 4
// == 0; an inward-shifted last window or a W that is not a multiple of 4 takes the scalar path for the affected
// quads).  The blend is a GATHER: the thread that owns an output pixel loops over the windows covering it in ascending
// plan order - no atomics, no dependence on the launch geometry, the same bits on every run.
#include "vu_common.h"
#include "vu_data.h"
#include "vu_tile_plan.h"
#include "../../include/vit_unet_amd.h"

namespace {

// one thread = 4 consecutive columns of one row of one window, all channels: CH bytes per pixel in, CH float4 out
template <int CH>
__global__ __launch_bounds__(256) void tile_gather_u8_kernel(const uint8_t* __restrict__ img, float* __restrict__ tiles, tile_axis Y,
                                                             tile_axis X, int t0, long long total, float m255, float rden, int vec) {
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= total) return;
  const int T = X.T, nq = (T + 3) >> 2;
  const int q = (int)(gid % nq);
  const long long r = gid / nq;
  const int y = (int)(r % T), w = (int)(r / T);
  const int t = t0 + w, x0 = q * 4;
  const int oy = axis_origin(Y, t / X.n), ox = axis_origin(X, t % X.n);
  const uint8_t* row = img + (size_t)axis_src(Y, oy + y) * X.L * CH;
  float v[CH][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (x0 + j < T) {
      const uint8_t* p = row + (size_t)axis_src(X, ox + x0 + j) * CH;
#pragma unroll
      for (int c = 0; c < CH; ++c) v[c][j] = vu_normalize_u8(p[c], m255, rden);
    }
  }
  const size_t plane = (size_t)T * T;
  float* o = tiles + (size_t)w * CH * plane + (size_t)y * T + x0;
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    if (vec) {
      *reinterpret_cast<float4*>(o + c * plane) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (x0 + j < T) o[c * plane + j] = v[c][j];
    }
  }
}

// one thread = 4 consecutive columns of one row of one channel of one window; values copied unchanged
__global__ __launch_bounds__(256) void tile_gather_f32_kernel(const float* __restrict__ img, float* __restrict__ tiles, tile_axis Y,
                                                              tile_axis X, int C, int t0, long long total, int vec_out, int vec_in) {
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= total) return;
  const int T = X.T, nq = (T + 3) >> 2;
  const int q = (int)(gid % nq);
  long long r = gid / nq;
  const int y = (int)(r % T);
  r /= T;
  const int c = (int)(r % C), w = (int)(r / C);
  const int t = t0 + w, x0 = q * 4;
  const int oy = axis_origin(Y, t / X.n), ox = axis_origin(X, t % X.n);
  const size_t rowoff = ((size_t)c * Y.L + axis_src(Y, oy + y)) * X.L;
  float v[4];
  // a quad that lies inside the image (no reflection) on a 16-byte boundary is one load
  if (vec_in && ox + x0 + 3 < X.L && ((rowoff + ox + x0) & 3) == 0) {
    const float4 f = *reinterpret_cast<const float4*>(img + rowoff + ox + x0);
    v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (x0 + j < T) v[j] = img[rowoff + axis_src(X, ox + x0 + j)];
  }
  float* o = tiles + (((size_t)w * C + c) * T + y) * T + x0;
  if (vec_out) {
    *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (x0 + j < T) o[j] = v[j];
  }
}

// one thread = 4 consecutive output pixels of one image row, all channels.  Per pixel: acc += w v, ws += w over the
// covering windows in ascending plan order (ty outer, tx inner), out = acc / ws; every operation rounded once, in float32.
template <int CH>
__global__ __launch_bounds__(256) void tile_blend_kernel(const float* __restrict__ tiles, float* __restrict__ out_f32,
                                                         uint8_t* __restrict__ out_u8, tile_axis Y, tile_axis X, long long total,
                                                         int vec_in, int vec_f32, int vec_u8) {
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= total) return;
  const int H = Y.L, W = X.L, T = X.T, nq = (W + 3) >> 2;
  const int y = (int)(gid / nq), x0 = (int)(gid % nq) * 4;
  const bool full = x0 + 3 < W;
  const size_t plane = (size_t)T * T;
  float acc[CH][4], ws[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    ws[j] = 0.f;
#pragma unroll
    for (int c = 0; c < CH; ++c) acc[c][j] = 0.f;
  }
  const int ix0 = axis_first(X, x0);
  for (int iy = axis_first(Y, y); iy < Y.n; ++iy) {
    const int oy = axis_origin(Y, iy);
    if (oy > y) break;
    const int ry = y - oy;
    if (ry >= T) continue;
    const float wy = axis_weight(Y, ry);
    for (int ix = ix0; ix < X.n; ++ix) {
      const int ox = axis_origin(X, ix);
      if (ox > x0 + 3) break;
      const int rx = x0 - ox;   // window column of the quad's first pixel; negative when the window starts inside the quad
      const float* p = tiles + (size_t)(iy * X.n + ix) * CH * plane + (size_t)ry * T;
      if (vec_in && full && rx >= 0 && rx + 3 < T && (rx & 3) == 0) {
        float w[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          w[j] = __fmul_rn(wy, axis_weight(X, rx + j));
          ws[j] = __fadd_rn(ws[j], w[j]);
        }
#pragma unroll
        for (int c = 0; c < CH; ++c) {
          const float4 f = *reinterpret_cast<const float4*>(p + c * plane + rx);
          acc[c][0] = __fadd_rn(acc[c][0], __fmul_rn(w[0], f.x));
          acc[c][1] = __fadd_rn(acc[c][1], __fmul_rn(w[1], f.y));
          acc[c][2] = __fadd_rn(acc[c][2], __fmul_rn(w[2], f.z));
          acc[c][3] = __fadd_rn(acc[c][3], __fmul_rn(w[3], f.w));
        }
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int rj = rx + j;
          if (rj >= 0 && rj < T && x0 + j < W) {
            const float w = __fmul_rn(wy, axis_weight(X, rj));
            ws[j] = __fadd_rn(ws[j], w);
#pragma unroll
            for (int c = 0; c < CH; ++c) acc[c][j] = __fadd_rn(acc[c][j], __fmul_rn(w, p[c * plane + rj]));
          }
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float d = x0 + j < W ? ws[j] : 1.f;
#pragma unroll
    for (int c = 0; c < CH; ++c) acc[c][j] = __fdiv_rn(acc[c][j], d);
  }
  if (out_f32) {
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const size_t o = ((size_t)c * H + y) * W + x0;
      if (vec_f32 && full && (o & 3) == 0) {
        *reinterpret_cast<float4*>(out_f32 + o) = make_float4(acc[c][0], acc[c][1], acc[c][2], acc[c][3]);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (x0 + j < W) out_f32[o + j] = acc[c][j];
      }
    }
  }
  if (out_u8) {
    uint8_t b[4 * CH];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int c = 0; c < CH; ++c)
        b[j * CH + c] = (uint8_t)fminf(fmaxf(floorf(__fadd_rn(__fmul_rn(255.f, acc[c][j]), 0.5f)), 0.f), 255.f);
    const size_t o = ((size_t)y * W + x0) * CH;
    if (vec_u8 && full && (o & 3) == 0) {   // 4 CH bytes = CH whole words
      uint32_t* d = reinterpret_cast<uint32_t*>(out_u8 + o);
#pragma unroll
      for (int k = 0; k < CH; ++k)
        d[k] = (uint32_t)b[4 * k] | ((uint32_t)b[4 * k + 1] << 8) | ((uint32_t)b[4 * k + 2] << 16) | ((uint32_t)b[4 * k + 3] << 24);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (x0 + j < W)
#pragma unroll
          for (int c = 0; c < CH; ++c) out_u8[o + j * CH + c] = b[j * CH + c];
    }
  }
}

int check_range(const char* who, const tile_axis& Y, const tile_axis& X, int C, int t0, int n) {
  VU_REQUIRE(C >= 1 && C <= 4, "%s: 1 to 4 channels (got %d)", who, C);
  VU_REQUIRE(t0 >= 0 && n > 0 && (long long)t0 + n <= (long long)Y.n * X.n,
             "%s: windows [%d, %d + %d) outside the plan of %d x %d windows", who, t0, t0, n, Y.n, X.n);
  return VU_OK;
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

inline bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + nb && b0 < a0 + na;
}

#define VU_TILE_BY_CH(C, KERNEL, ...)                                                           \
  switch (C) {                                                                                   \
    case 1: hipLaunchKernelGGL(KERNEL<1>, grid, dim3(256), 0, st, __VA_ARGS__); break;           \
    case 2: hipLaunchKernelGGL(KERNEL<2>, grid, dim3(256), 0, st, __VA_ARGS__); break;           \
    case 3: hipLaunchKernelGGL(KERNEL<3>, grid, dim3(256), 0, st, __VA_ARGS__); break;           \
    default: hipLaunchKernelGGL(KERNEL<4>, grid, dim3(256), 0, st, __VA_ARGS__); break;          \
  }

}  // namespace

extern "C" {

int vu_tile_plan_axis(int L, int T, int overlap, int* origins, int capacity) {
  int rc = check_plan("tile_plan_axis", L, L, T, overlap);
  if (rc) return rc;
  const tile_axis a = make_axis(L, T, overlap);
  VU_REQUIRE(origins && capacity >= a.n, "tile_plan_axis: %d windows do not fit a capacity of %d", a.n, origins ? capacity : 0);
  for (int i = 0; i < a.n; ++i) origins[i] = axis_origin(a, i);
  return a.n;
}

int vu_tile_plan_count(int H, int W, int T, int overlap, int* ny, int* nx) {
  int rc = check_plan("tile_plan_count", H, W, T, overlap);
  if (rc) return rc;
  VU_REQUIRE(ny && nx, "tile_plan_count: null argument");
  const long long y = axis_count(H, T, T - overlap), x = axis_count(W, T, T - overlap);
  VU_REQUIRE(y * x <= 0x7fffffffLL, "tile_plan_count: %lld x %lld windows exceed the int range", y, x);
  *ny = (int)y;
  *nx = (int)x;
  return VU_OK;
}

int vu_tile_gather_u8(const uint8_t* img, float* tiles, int H, int W, int C, int T, int overlap, int t0, int n, float mean,
                      float std, void* stream) {
  int rc = check_plan("tile_gather_u8", H, W, T, overlap);
  if (rc) return rc;
  const tile_axis Y = make_axis(H, T, overlap), X = make_axis(W, T, overlap);
  if ((rc = check_range("tile_gather_u8", Y, X, C, t0, n))) return rc;
  VU_REQUIRE(img && tiles, "tile_gather_u8: null argument");
  VU_REQUIRE(std > 0.f, "tile_gather_u8: std must be positive");
  const long long total = (long long)n * T * ((T + 3) / 4);
  VU_REQUIRE(vu_cdiv64(total, 256) <= 0x7fffffffLL, "tile_gather_u8: launch too large (%d windows of %d)", n, T);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)vu_cdiv64(total, 256));
  const int vec = (T % 4 == 0 && aligned16(tiles)) ? 1 : 0;
  const float m255 = vu_normalize_m255(mean), rden = vu_normalize_rden(std);
  VU_TILE_BY_CH(C, tile_gather_u8_kernel, img, tiles, Y, X, t0, total, m255, rden, vec);
  if (vu_prof_on()) vu_prof_note("tile_gather_u8_kernel", 0.0, (double)H * W * C + 4.0 * n * C * T * T);
  return vu_check_launch("vu_tile_gather_u8");
}

int vu_tile_gather_f32(const float* img, float* tiles, int H, int W, int C, int T, int overlap, int t0, int n, void* stream) {
  int rc = check_plan("tile_gather_f32", H, W, T, overlap);
  if (rc) return rc;
  const tile_axis Y = make_axis(H, T, overlap), X = make_axis(W, T, overlap);
  if ((rc = check_range("tile_gather_f32", Y, X, C, t0, n))) return rc;
  VU_REQUIRE(img && tiles, "tile_gather_f32: null argument");
  const long long total = (long long)n * C * T * ((T + 3) / 4);
  VU_REQUIRE(vu_cdiv64(total, 256) <= 0x7fffffffLL, "tile_gather_f32: launch too large (%d windows of %d)", n, T);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)vu_cdiv64(total, 256));
  const int vec_out = (T % 4 == 0 && aligned16(tiles)) ? 1 : 0, vec_in = aligned16(img) ? 1 : 0;
  hipLaunchKernelGGL(tile_gather_f32_kernel, grid, dim3(256), 0, st, img, tiles, Y, X, C, t0, total, vec_out, vec_in);
  if (vu_prof_on()) vu_prof_note("tile_gather_f32_kernel", 0.0, 4.0 * H * W * C + 4.0 * n * C * T * T);
  return vu_check_launch("vu_tile_gather_f32");
}

int vu_tile_blend(const float* tiles, float* out_f32, uint8_t* out_u8, int H, int W, int C, int T, int overlap, void* stream) {
  int rc = check_plan("tile_blend", H, W, T, overlap);
  if (rc) return rc;
  const tile_axis Y = make_axis(H, T, overlap), X = make_axis(W, T, overlap);
  VU_REQUIRE(C >= 1 && C <= 4, "tile_blend: 1 to 4 channels (got %d)", C);
  VU_REQUIRE((long long)Y.n * X.n <= 0x7fffffffLL, "tile_blend: %d x %d windows exceed the int range", Y.n, X.n);
  VU_REQUIRE(tiles && (out_f32 || out_u8), "tile_blend: null argument (windows, and at least one of out_f32 / out_u8)");
  const size_t tile_bytes = (size_t)Y.n * X.n * C * T * T * 4, px = (size_t)H * W * C;
  VU_REQUIRE(!(out_f32 && ranges_overlap(tiles, tile_bytes, out_f32, px * 4)) && !(out_u8 && ranges_overlap(tiles, tile_bytes, out_u8, px)),
             "tile_blend: the output must not alias the window buffer");
  const long long total = (long long)H * ((W + 3) / 4);
  VU_REQUIRE(vu_cdiv64(total, 256) <= 0x7fffffffLL, "tile_blend: launch too large (%d x %d)", H, W);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)vu_cdiv64(total, 256));
  const int vec_in = (T % 4 == 0 && aligned16(tiles)) ? 1 : 0, vec_f32 = (out_f32 && aligned16(out_f32)) ? 1 : 0;
  const int vec_u8 = (out_u8 && ((uintptr_t)out_u8 & 3) == 0) ? 1 : 0;
  VU_TILE_BY_CH(C, tile_blend_kernel, tiles, out_f32, out_u8, Y, X, total, vec_in, vec_f32, vec_u8);
  if (vu_prof_on()) vu_prof_note("tile_blend_kernel", 0.0, 4.0 * Y.n * X.n * C * T * T + (out_f32 ? 4.0 : 0.0) * px + (out_u8 ? 1.0 : 0.0) * px);
  return vu_check_launch("vu_tile_blend");
}

}  // extern "C"
