// Whole-slice / volume segmentation: the segmentation twin of csrc/vu_tile.hip.  A (D,H,W) int16 volume (one slice: D = 1) is
// covered slice by slice with the window plan of csrc/vu_tile_plan.h; windows are numbered over the whole volume, g = z nt + t
// (nt = ny nx windows per slice).  vu_tile_gather_i16 cuts windows [g0, g0 + n) into the (n,1,T,T) batch the eval forward takes,
// under the intensity window of the segmentation input pipeline (csrc/vu_data.h: vu_window_i16, what vu_seg_prepare applies);
// vu_seg_blend puts the window outputs (logits) of nz consecutive slices back together with exactly the arithmetic of
// vu_tile_blend at C = 1 and ends in what a segmentation user wants: the blended logit, the thresholded mask and, against a
// truth volume, the three integer counts per slice that Dice and IoU are made of.
//
// Both kernels are pure streaming, one thread = 4 consecutive pixels of a row: an 8-byte int16 load / a 16-byte float store in
// the gather, 16-byte window reads and logit stores and 4-byte mask stores / truth loads in the blend wherever the addresses allow
// it, guarded scalar accesses elsewhere (partial quads, reflection, inward-shifted windows, odd W, unaligned buffers).
// The counts are integers: per-block partial counts (uint32, a block owns at most 1024 pixels) go to `scratch`, a second kernel
// sums them per slice in a fixed order into uint64 - exact whatever the launch geometry, no atomics.
#include "vu_common.h"
#include "vu_data.h"
#include "vu_tile_plan.h"
#include "../../include/vit_unet_amd.h"

namespace {

// one thread = 4 consecutive columns of one row of one window
__global__ __launch_bounds__(256) void tile_gather_i16_kernel(const int16_t* __restrict__ vol, float* __restrict__ tiles, tile_axis Y,
                                                              tile_axis X, long long g0, long long total, float lo, float range,
                                                              int vec_out) {
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= total) return;
  const int T = X.T, nq = (T + 3) >> 2, nt = Y.n * X.n;
  const int q = (int)(gid % nq);
  const long long r = gid / nq;
  const int y = (int)(r % T);
  const long long w = r / T, g = g0 + w;
  const long long z = g / nt;
  const int t = (int)(g % nt), x0 = q * 4;
  const int oy = axis_origin(Y, t / X.n), ox = axis_origin(X, t % X.n);
  const int16_t* row = vol + ((size_t)z * Y.L + axis_src(Y, oy + y)) * X.L;
  int v[4] = {0, 0, 0, 0};
  // a quad that lies inside the slice (no reflection) on an 8-byte boundary is one load; with an odd W every other row is not
  if (ox + x0 + 3 < X.L && ((uintptr_t)(row + ox + x0) & 7) == 0) {
    const s16x4 s = *reinterpret_cast<const s16x4*>(row + ox + x0);
    v[0] = s.x; v[1] = s.y; v[2] = s.z; v[3] = s.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (x0 + j < T) v[j] = row[axis_src(X, ox + x0 + j)];
  }
  float* o = tiles + ((size_t)w * T + y) * T + x0;
  if (vec_out) {
    *reinterpret_cast<float4*>(o) = make_float4(vu_window_i16(v[0], lo, range), vu_window_i16(v[1], lo, range),
                                                vu_window_i16(v[2], lo, range), vu_window_i16(v[3], lo, range));
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (x0 + j < T) o[j] = vu_window_i16(v[j], lo, range);
  }
}

__device__ __forceinline__ unsigned wave_sum_u32(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// one thread = 4 consecutive output pixels of one row of one slice; blockIdx.x = slice * nb + block of the slice.  The logit is
// tile_blend_kernel<1>'s: acc += w v, ws += w over the covering windows in ascending plan order, z = acc / ws, every operation
// rounded once in float32.  label < 0: a truth pixel is truth != 0, else truth == label.
__global__ __launch_bounds__(256) void seg_blend_kernel(const float* __restrict__ tiles, const uint8_t* __restrict__ truth,
                                                        float* __restrict__ logits, uint8_t* __restrict__ mask,
                                                        uint32_t* __restrict__ partials, tile_axis Y, tile_axis X, int nb, int per_slice,
                                                        float zthr, int label, int vec_in, int vec_f32, int vec_mask, int vec_truth) {
  __shared__ unsigned sm[2][4];
  const int zs = blockIdx.x / nb, bs = blockIdx.x % nb;
  const int lid = bs * 256 + threadIdx.x;
  unsigned c_pred = 0, c_true = 0, c_both = 0;
  if (lid < per_slice) {
    const int H = Y.L, W = X.L, T = X.T, nq = (W + 3) >> 2;
    const int y = lid / nq, x0 = (lid % nq) * 4;
    const bool full = x0 + 3 < W;
    const size_t plane = (size_t)T * T;
    const float* slice_tiles = tiles + (size_t)zs * Y.n * X.n * plane;
    float acc[4], ws[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) { ws[j] = 0.f; acc[j] = 0.f; }
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
        const float* p = slice_tiles + (size_t)(iy * X.n + ix) * plane + (size_t)ry * T;
        if (vec_in && full && rx >= 0 && rx + 3 < T && (rx & 3) == 0) {
          float w[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            w[j] = __fmul_rn(wy, axis_weight(X, rx + j));
            ws[j] = __fadd_rn(ws[j], w[j]);
          }
          const float4 f = *reinterpret_cast<const float4*>(p + rx);
          acc[0] = __fadd_rn(acc[0], __fmul_rn(w[0], f.x));
          acc[1] = __fadd_rn(acc[1], __fmul_rn(w[1], f.y));
          acc[2] = __fadd_rn(acc[2], __fmul_rn(w[2], f.z));
          acc[3] = __fadd_rn(acc[3], __fmul_rn(w[3], f.w));
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int rj = rx + j;
            if (rj >= 0 && rj < T && x0 + j < W) {
              const float w = __fmul_rn(wy, axis_weight(X, rj));
              ws[j] = __fadd_rn(ws[j], w);
              acc[j] = __fadd_rn(acc[j], __fmul_rn(w, p[rj]));
            }
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = __fdiv_rn(acc[j], x0 + j < W ? ws[j] : 1.f);
    const size_t o = ((size_t)zs * H + y) * W + x0;
    if (logits) {
      if (vec_f32 && full && (o & 3) == 0) {
        *reinterpret_cast<float4*>(logits + o) = make_float4(acc[0], acc[1], acc[2], acc[3]);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (x0 + j < W) logits[o + j] = acc[j];
      }
    }
    unsigned m[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) m[j] = (x0 + j < W && acc[j] >= zthr) ? 1u : 0u;
    if (mask) {
      if (vec_mask && full && (o & 3) == 0) {
        *reinterpret_cast<uint32_t*>(mask + o) = m[0] | (m[1] << 8) | (m[2] << 16) | (m[3] << 24);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (x0 + j < W) mask[o + j] = (uint8_t)m[j];
      }
    }
    if (partials) {
      unsigned tv[4] = {0u, 0u, 0u, 0u};
      if (vec_truth && full && (o & 3) == 0) {
        const uint32_t u = *reinterpret_cast<const uint32_t*>(truth + o);
        tv[0] = u & 255u; tv[1] = (u >> 8) & 255u; tv[2] = (u >> 16) & 255u; tv[3] = u >> 24;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (x0 + j < W) tv[j] = truth[o + j];
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const unsigned tj = (x0 + j < W && (label < 0 ? tv[j] != 0u : tv[j] == (unsigned)label)) ? 1u : 0u;
        c_pred += m[j]; c_true += tj; c_both += m[j] & tj;
      }
    }
  }
  if (!partials) return;   // the same in every thread of the launch
  // a block owns at most 1024 pixels: pred and both share one word (16 bits each)
  const unsigned a = wave_sum_u32(c_pred | (c_both << 16)), b = wave_sum_u32(c_true);
  const int wv = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { sm[0][wv] = a; sm[1][wv] = b; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned sa = sm[0][0] + sm[0][1] + sm[0][2] + sm[0][3], sb = sm[1][0] + sm[1][1] + sm[1][2] + sm[1][3];
    uint32_t* d = partials + (size_t)blockIdx.x * 3;
    d[0] = sa & 0xffffu; d[1] = sb; d[2] = sa >> 16;
  }
}

// one block per slice: thread i sums partials i, i + 256, ..., then a fixed tree over the 256 threads
__global__ __launch_bounds__(256) void seg_counts_kernel(const uint32_t* __restrict__ partials, unsigned long long* __restrict__ counts,
                                                         int nb) {
  __shared__ unsigned long long sd[3][256];
  const uint32_t* p = partials + (size_t)blockIdx.x * nb * 3;
  unsigned long long a = 0, b = 0, c = 0;
  for (int i = threadIdx.x; i < nb; i += 256) { a += p[3 * i]; b += p[3 * i + 1]; c += p[3 * i + 2]; }
  sd[0][threadIdx.x] = a; sd[1][threadIdx.x] = b; sd[2][threadIdx.x] = c;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o)
      for (int q = 0; q < 3; ++q) sd[q][threadIdx.x] += sd[q][threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x < 3) counts[(size_t)blockIdx.x * 3 + threadIdx.x] = sd[threadIdx.x][0];
}

inline bool aligned_to(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

inline bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + nb && b0 < a0 + na;
}

inline long long blocks_per_slice(int H, int W) { return vu_cdiv64((long long)H * ((W + 3) / 4), 256); }

}  // namespace

extern "C" {

int vu_tile_gather_i16(const int16_t* vol, float* tiles, int D, int H, int W, int T, int overlap, long long g0, int n, float lo,
                       float hi, void* stream) {
  int rc = check_plan("tile_gather_i16", H, W, T, overlap);
  if (rc) return rc;
  VU_REQUIRE(D > 0, "tile_gather_i16: empty volume (%d slices)", D);
  const tile_axis Y = make_axis(H, T, overlap), X = make_axis(W, T, overlap);
  const long long nt = (long long)Y.n * X.n;
  VU_REQUIRE(nt <= 0x7fffffffLL, "tile_gather_i16: %d x %d windows exceed the int range", Y.n, X.n);
  VU_REQUIRE(g0 >= 0 && n > 0 && g0 + n <= (long long)D * nt,
             "tile_gather_i16: windows [%lld, %lld + %d) outside the plan of %d slices of %lld windows", g0, g0, n, D, nt);
  VU_REQUIRE(vol && tiles, "tile_gather_i16: null argument");
  VU_REQUIRE(hi > lo, "tile_gather_i16: intensity window must have hi > lo (got %g..%g)", (double)lo, (double)hi);
  const long long total = (long long)n * T * ((T + 3) / 4);
  VU_REQUIRE(vu_cdiv64(total, 256) <= 0x7fffffffLL, "tile_gather_i16: launch too large (%d windows of %d)", n, T);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)vu_cdiv64(total, 256));
  const int vec_out = (T % 4 == 0 && aligned_to(tiles, 16)) ? 1 : 0;
  hipLaunchKernelGGL(tile_gather_i16_kernel, grid, dim3(256), 0, st, vol, tiles, Y, X, g0, total, lo, hi - lo, vec_out);
  if (vu_prof_on()) vu_prof_note("tile_gather_i16_kernel", 0.0, 6.0 * n * T * T);
  return vu_check_launch("vu_tile_gather_i16");
}

size_t vu_seg_blend_scratch_bytes(int nz, int H, int W) {
  if (nz <= 0 || H <= 0 || W <= 0) return 0;
  return (size_t)nz * (size_t)blocks_per_slice(H, W) * 3 * sizeof(uint32_t);
}

int vu_seg_blend(const float* tiles, const uint8_t* truth, float* logits, uint8_t* mask, unsigned long long* counts, void* scratch,
                 size_t scratch_bytes, int nz, int H, int W, int T, int overlap, float zthr, int label, void* stream) {
  int rc = check_plan("seg_blend", H, W, T, overlap);
  if (rc) return rc;
  VU_REQUIRE(nz > 0, "seg_blend: no slice (nz = %d)", nz);
  VU_REQUIRE(label <= 255, "seg_blend: label must be negative (any non-zero truth) or 0 .. 255 (got %d)", label);
  VU_REQUIRE(zthr == zthr, "seg_blend: the threshold is not a number");
  const tile_axis Y = make_axis(H, T, overlap), X = make_axis(W, T, overlap);
  const long long nt = (long long)Y.n * X.n;
  VU_REQUIRE(nt <= 0x7fffffffLL, "seg_blend: %d x %d windows exceed the int range", Y.n, X.n);
  VU_REQUIRE(tiles && (logits || mask || counts), "seg_blend: null argument (windows, and at least one of logits / mask / counts)");
  VU_REQUIRE(!counts || truth, "seg_blend: counts need a truth volume");
  const long long nb = blocks_per_slice(H, W), per_slice = (long long)H * ((W + 3) / 4);
  VU_REQUIRE(per_slice <= 0x7fffffffLL && nb * nz <= 0x7fffffffLL, "seg_blend: launch too large (%d slices of %d x %d)", nz, H, W);
  const size_t tile_bytes = (size_t)nz * nt * T * T * 4, px = (size_t)nz * H * W;
  VU_REQUIRE(!(logits && ranges_overlap(tiles, tile_bytes, logits, px * 4)) && !(mask && ranges_overlap(tiles, tile_bytes, mask, px)) &&
                 !(counts && ranges_overlap(tiles, tile_bytes, counts, (size_t)nz * 24)),
             "seg_blend: the outputs must not alias the window buffer");
  if (counts) {
    const size_t need = vu_seg_blend_scratch_bytes(nz, H, W);
    VU_REQUIRE(scratch && scratch_bytes >= need && aligned_to(scratch, 4), "seg_blend: scratch too small or misaligned (%zu bytes needed)", need);
    VU_REQUIRE(aligned_to(counts, 8), "seg_blend: counts must be 8-byte aligned");
    VU_REQUIRE(!ranges_overlap(tiles, tile_bytes, scratch, need), "seg_blend: the scratch must not alias the window buffer");
  }
  hipStream_t st = (hipStream_t)stream;
  const int vec_in = (T % 4 == 0 && aligned_to(tiles, 16)) ? 1 : 0, vec_f32 = (logits && aligned_to(logits, 16)) ? 1 : 0;
  const int vec_mask = (mask && aligned_to(mask, 4)) ? 1 : 0, vec_truth = (counts && aligned_to(truth, 4)) ? 1 : 0;
  hipLaunchKernelGGL(seg_blend_kernel, dim3((unsigned)(nb * nz)), dim3(256), 0, st, tiles, truth, logits, mask,
                     counts ? (uint32_t*)scratch : (uint32_t*)nullptr, Y, X, (int)nb, (int)per_slice, zthr, label, vec_in, vec_f32,
                     vec_mask, vec_truth);
  if (vu_prof_on())
    vu_prof_note("seg_blend_kernel", 0.0, 4.0 * nz * nt * T * T + ((logits ? 4.0 : 0.0) + (mask ? 1.0 : 0.0) + (counts ? 1.0 : 0.0)) * px);
  rc = vu_check_launch("vu_seg_blend");
  if (rc || !counts) return rc;
  hipLaunchKernelGGL(seg_counts_kernel, dim3(nz), dim3(256), 0, st, (const uint32_t*)scratch, counts, (int)nb);
  return vu_check_launch("vu_seg_blend/counts");
}

}  // extern "C"
