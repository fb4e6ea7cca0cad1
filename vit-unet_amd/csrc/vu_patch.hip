// Native-resolution training patches and the x8 self-ensemble: both rest on one primitive, a dihedral transform of a
// T x T window.  op in 0..7: k = op & 3 counter-clockwise quarter turns, applied after a left-right flip when op & 4:
//   D_op(p) = np.rot90(np.fliplr(p) if op & 4 else p, k = op & 3)
// Output pixel (i, j) of D_op comes from source pixel (sy, sx):
//   even k (rows stay rows):       sy = fy ? T-1-i : i,   sx = fx ? T-1-j : j
//   odd  k (a transpose is part):  sy = fy ? T-1-j : j,   sx = fx ? T-1-i : i
// with fy = k >= 2 and fx = (k == 1 || k == 2) xor flip:
//   op   0      1        2          3        4        5      6        7
//   src  (i,j)  (j,T-1-i) (T-1-i,T-1-j) (T-1-j,i) (i,T-1-j) (j,i) (T-1-i,j) (T-1-j,T-1-i)
// The inverse of an op is an op (vu_dihedral_inverse), so the kernels know the forward mapping only.
//
//   vu_patch_pairs_u8   cuts n crops (y0, x0, op) out of one decoded noisy / clean uint8 HWC pair and stores D_op of each as
//                       (n,C,T,T) float32 under the validation transform (csrc/vu_data.h: the arithmetic of vu_denoise_prepare)
//   vu_dihedral_f32     D_op of every plane of an (n,C,T,T) float32 batch, optionally added to the destination and scaled
//
// Access pattern.  A block owns one 32 x 32 tile of one output plane (of all C planes of a crop in the u8 kernel), one thread
// = 4 consecutive output columns of one row: stores (and the accumulate reads) run along rows, 16 bytes per lane where T % 4
// == 0 and the buffer is 16-byte aligned, scalar otherwise.  With even k the source quad of a thread is a plain or a reversed
// run of one source row and is read directly.  With odd k the output ROW index walks along a source ROW, so a direct read
// would put neighbouring lanes a whole source row apart; instead the 32 x 32 source tile is read along ITS rows into LDS
// ([32][33] dwords: the pad makes the row-wise fill and the column-wise drain both conflict-free over the 32 banks that
// 4-byte LDS accesses use; the u8 kernel packs the <= 4 channel bytes of a pixel into one dword) and drained transposed.
// Tiles at the patch edge are partial: every access is guarded by i < T / j < T.  No atomics: the same bits on every run.
#include "vu_common.h"
#include "vu_data.h"
#include "../../include/vit_unet_amd.h"

namespace {

constexpr int TS = 32;   // tile side; 256 threads = 32 rows x 8 quads

struct dihedral_map {
  int tr, fy, fx;
};

__host__ __device__ __forceinline__ dihedral_map make_map(int op) {
  const int k = op & 3;
  dihedral_map m;
  m.tr = k & 1;
  m.fy = k >> 1;
  m.fx = ((k ^ (k >> 1)) & 1) ^ ((op >> 2) & 1);
  return m;
}

__device__ __forceinline__ int flip_if(int f, int T, int v) { return f ? T - 1 - v : v; }

// one block = one 32 x 32 tile of one (T,T) plane; one op for the whole launch, so the transposing form is a template argument
template <bool TR>
__global__ __launch_bounds__(256) void dihedral_f32_kernel(const float* __restrict__ src, float* __restrict__ dst, int T, int nt,
                                                           int fy, int fx, int accumulate, float scale, int vec) {
  __shared__ float lds[TR ? TS : 1][TS + 1];
  const int per = nt * nt;
  const size_t plane = (size_t)(blockIdx.x / per) * T * T;
  const int tile = blockIdx.x % per;
  const int i0 = (tile / nt) * TS, j0 = (tile % nt) * TS;
  const int r = threadIdx.x >> 3, q4 = (threadIdx.x & 7) * 4;
  const float* s = src + plane;
  float v[4];
  if (TR) {
    // fill: lds[r][c] = D_op value of output pixel (i0 + c, j0 + r); the quad runs along source columns
    const int j = j0 + r, i = i0 + q4;
    if (j < T && i < T) {
      const float* row = s + (size_t)flip_if(fy, T, j) * T;
      if (vec) {   // T % 4 == 0: the quad lies inside the plane, on a 16-byte boundary in either direction
        const float4 f = *reinterpret_cast<const float4*>(row + (fx ? T - 4 - i : i));
        lds[r][q4 + 0] = fx ? f.w : f.x;
        lds[r][q4 + 1] = fx ? f.z : f.y;
        lds[r][q4 + 2] = fx ? f.y : f.z;
        lds[r][q4 + 3] = fx ? f.x : f.w;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (i + e < T) lds[r][q4 + e] = row[flip_if(fx, T, i + e)];
      }
    }
    __syncthreads();
  }
  const int i = i0 + r, j = j0 + q4;
  if (i >= T || j >= T) return;
  if (TR) {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (j + e < T) v[e] = lds[q4 + e][r];
  } else {
    const float* row = s + (size_t)flip_if(fy, T, i) * T;
    if (vec) {
      const float4 f = *reinterpret_cast<const float4*>(row + (fx ? T - 4 - j : j));
      v[0] = fx ? f.w : f.x;
      v[1] = fx ? f.z : f.y;
      v[2] = fx ? f.y : f.z;
      v[3] = fx ? f.x : f.w;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (j + e < T) v[e] = row[flip_if(fx, T, j + e)];
    }
  }
  float* o = dst + plane + (size_t)i * T + j;
  if (vec) {
    if (accumulate) {
      const float4 a = *reinterpret_cast<const float4*>(o);
      v[0] = __fadd_rn(a.x, v[0]);
      v[1] = __fadd_rn(a.y, v[1]);
      v[2] = __fadd_rn(a.z, v[2]);
      v[3] = __fadd_rn(a.w, v[3]);
    }
    if (scale != 1.f) {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = __fmul_rn(v[e], scale);
    }
    *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (j + e < T) {
        float t = accumulate ? __fadd_rn(o[e], v[e]) : v[e];
        if (scale != 1.f) t = __fmul_rn(t, scale);
        o[e] = t;
      }
    }
  }
}

template <int CH>
__device__ __forceinline__ uint32_t load_px(const uint8_t* __restrict__ p) {
  uint32_t w = 0;
#pragma unroll
  for (int c = 0; c < CH; ++c) w |= (uint32_t)p[c] << (8 * c);
  return w;
}

// one block = one 32 x 32 tile of one crop, both images, all channels.  The op is per crop (table in device memory), so the
// choice between the direct and the transposing form is a branch that is uniform over the block.
template <int CH>
__global__ __launch_bounds__(256) void patch_pairs_kernel(const uint8_t* __restrict__ noisy, const uint8_t* __restrict__ clean,
                                                          float* __restrict__ x, float* __restrict__ y, int H, int W, int T, int nt,
                                                          const int* __restrict__ crops, float m255, float rden, int vecx, int vecy) {
  __shared__ uint32_t ldn[TS][TS + 1], ldc[TS][TS + 1];
  const int per = nt * nt;
  const int crop = blockIdx.x / per, tile = blockIdx.x % per;
  const int i0 = (tile / nt) * TS, j0 = (tile % nt) * TS;
  // the table is device data the host never saw: clamp, so that no content can make the kernel read outside the image
  const int* ct = crops + (size_t)3 * crop;
  const int y0 = min(max(ct[0], 0), H - T), x0 = min(max(ct[1], 0), W - T);
  const dihedral_map m = make_map(ct[2] & 7);
  const int r = threadIdx.x >> 3, q4 = (threadIdx.x & 7) * 4;
  uint32_t pn[4] = {0u, 0u, 0u, 0u}, pc[4] = {0u, 0u, 0u, 0u};
  if (m.tr) {
    // fill along source rows: lane c of a 32-lane half = source column of output row i0 + c, 4 passes of 8 source rows
    const int c = threadIdx.x & 31, i = i0 + c;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int rr = (threadIdx.x >> 5) + 8 * k, j = j0 + rr;
      if (i < T && j < T) {
        const size_t off = ((size_t)(y0 + flip_if(m.fy, T, j)) * W + x0 + flip_if(m.fx, T, i)) * CH;
        if (noisy) ldn[rr][c] = load_px<CH>(noisy + off);
        if (clean) ldc[rr][c] = load_px<CH>(clean + off);
      }
    }
    __syncthreads();
  }
  const int i = i0 + r, j = j0 + q4;
  if (i >= T || j >= T) return;
  if (m.tr) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (j + e < T) {
        if (noisy) pn[e] = ldn[q4 + e][r];
        if (clean) pc[e] = ldc[q4 + e][r];
      }
    }
  } else {
    const size_t row = (size_t)(y0 + flip_if(m.fy, T, i)) * W + x0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (j + e < T) {
        const size_t off = (row + flip_if(m.fx, T, j + e)) * CH;
        if (noisy) pn[e] = load_px<CH>(noisy + off);
        if (clean) pc[e] = load_px<CH>(clean + off);
      }
    }
  }
  const size_t plane = (size_t)T * T, base = (size_t)crop * CH * plane + (size_t)i * T + j;
  if (noisy) {
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      float v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = vu_normalize_u8((int)((pn[e] >> (8 * c)) & 255u), m255, rden);
      float* o = x + base + c * plane;
      if (vecx) {
        *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (j + e < T) o[e] = v[e];
      }
    }
  }
  if (clean) {
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      float v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = vu_unit_u8((int)((pc[e] >> (8 * c)) & 255u));
      float* o = y + base + c * plane;
      if (vecy) {
        *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (j + e < T) o[e] = v[e];
      }
    }
  }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

inline bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + nb && b0 < a0 + na;
}

}  // namespace

extern "C" {

int vu_dihedral_inverse(int op) {
  if (op < 0 || op > 7) return VU_EINVAL;
  return (op & 4) ? op : ((4 - op) & 3);
}

int vu_patch_pairs_u8(const uint8_t* noisy, const uint8_t* clean, float* x, float* y, int H, int W, int C, int T, const int* crops,
                      int n, float mean, float std, void* stream) {
  VU_REQUIRE(C >= 1 && C <= 4, "patch_pairs_u8: 1 to 4 channels (got %d)", C);
  VU_REQUIRE(T >= 1, "patch_pairs_u8: the patch size must be positive (got %d)", T);
  VU_REQUIRE(H >= T && W >= T, "patch_pairs_u8: a %d x %d image is smaller than a patch of %d (small images are refused, not reflected)",
             H, W, T);
  VU_REQUIRE(n >= 1, "patch_pairs_u8: no crop (n = %d)", n);
  VU_REQUIRE(std > 0.f, "patch_pairs_u8: std must be positive");
  VU_REQUIRE((noisy && x) || (clean && y), "patch_pairs_u8: null argument: nothing to do (no noisy/x and no clean/y pair)");
  VU_REQUIRE((noisy == nullptr) == (x == nullptr) && (clean == nullptr) == (y == nullptr),
             "patch_pairs_u8: null argument: input and output of a pair must both be given");
  VU_REQUIRE(crops, "patch_pairs_u8: null argument (the crop table)");
  const int nt = vu_cdiv(T, TS);
  const long long blocks = (long long)n * nt * nt;
  VU_REQUIRE(blocks <= 0x7fffffffLL, "patch_pairs_u8: launch too large (%d crops of %d)", n, T);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)blocks);
  const int vecx = (x && T % 4 == 0 && aligned16(x)) ? 1 : 0, vecy = (y && T % 4 == 0 && aligned16(y)) ? 1 : 0;
  const float m255 = vu_normalize_m255(mean), rden = vu_normalize_rden(std);
  switch (C) {
    case 1: hipLaunchKernelGGL(patch_pairs_kernel<1>, grid, dim3(256), 0, st, noisy, clean, x, y, H, W, T, nt, crops, m255, rden, vecx, vecy); break;
    case 2: hipLaunchKernelGGL(patch_pairs_kernel<2>, grid, dim3(256), 0, st, noisy, clean, x, y, H, W, T, nt, crops, m255, rden, vecx, vecy); break;
    case 3: hipLaunchKernelGGL(patch_pairs_kernel<3>, grid, dim3(256), 0, st, noisy, clean, x, y, H, W, T, nt, crops, m255, rden, vecx, vecy); break;
    default: hipLaunchKernelGGL(patch_pairs_kernel<4>, grid, dim3(256), 0, st, noisy, clean, x, y, H, W, T, nt, crops, m255, rden, vecx, vecy); break;
  }
  if (vu_prof_on()) vu_prof_note("patch_pairs_kernel", 0.0, 5.0 * n * C * T * T * ((noisy ? 1 : 0) + (clean ? 1 : 0)) + 12.0 * n);
  return vu_check_launch("vu_patch_pairs_u8");
}

int vu_dihedral_f32(const float* src, float* dst, int n, int C, int T, int op, int accumulate, float scale, void* stream) {
  VU_REQUIRE(n >= 1 && C >= 1 && T >= 1, "dihedral_f32: empty batch (n %d, C %d, T %d)", n, C, T);
  VU_REQUIRE(op >= 0 && op <= 7, "dihedral_f32: op must be in 0 .. 7 (got %d)", op);
  VU_REQUIRE(src && dst, "dihedral_f32: null argument");
  const size_t bytes = (size_t)n * C * T * T * 4;
  VU_REQUIRE(!ranges_overlap(src, bytes, dst, bytes), "dihedral_f32: dst must not overlap src (the transform is not done in place)");
  const int nt = vu_cdiv(T, TS);
  const long long blocks = (long long)n * C * nt * nt;
  VU_REQUIRE(blocks <= 0x7fffffffLL, "dihedral_f32: launch too large (%d x %d planes of %d)", n, C, T);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)blocks);
  const dihedral_map m = make_map(op);
  const int vec = (T % 4 == 0 && aligned16(src) && aligned16(dst)) ? 1 : 0, acc = accumulate ? 1 : 0;
  if (m.tr) hipLaunchKernelGGL(dihedral_f32_kernel<true>, grid, dim3(256), 0, st, src, dst, T, nt, m.fy, m.fx, acc, scale, vec);
  else hipLaunchKernelGGL(dihedral_f32_kernel<false>, grid, dim3(256), 0, st, src, dst, T, nt, m.fy, m.fx, acc, scale, vec);
  if (vu_prof_on()) vu_prof_note("dihedral_f32_kernel", 0.0, (accumulate ? 3.0 : 2.0) * (double)bytes);
  return vu_check_launch("vu_dihedral_f32");
}

}  // extern "C"
