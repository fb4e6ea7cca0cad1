// Volume resampling to a working spacing and back: (Di,Hi,Wi) -> (Do,Ho,Wo) with half-pixel centres and replicated edges, driven by
// the two shapes alone (a spacing exists only in Python).  Three entries: int16 trilinear (the image), uint8 nearest (label masks)
// and float32 trilinear that ends in the thresholded mask and the per-slice overlap counts (logits on their way back to the native
// grid).  The arithmetic is the contract of include/vit_unet_amd.h: exact integer tap tables with Q = 2^15, stages x, then y, then z,
// every rounding stated, so that a numpy restatement gives the same bits.
//
// One workgroup of 256 threads owns a tile of RS_TX x RS_TY outputs of one slice (RS_TZ = 1); one thread = 4 consecutive x outputs of
// one row.  The taps of the tile (RS_TX along x, RS_TY along y, one along z) are computed once per workgroup into LDS - the 64-bit
// divisions of the table rule run once per tap, not per voxel - and every output is then fused in registers: 4 x-stages, 2 y-stages
// and 1 z-stage, the same bits as three passes.  Stores are 8 (int16), 16 (float32) or 4 (uint8) bytes per thread where Wo % 4 == 0
// and the buffer is aligned, guarded scalar accesses elsewhere; the source taps are scalar gathers served by the caches.
// The counts are integers: per-workgroup partial counts (uint32; a workgroup owns 1024 pixels) go to `scratch`, a second launch sums
// them per slice in a fixed order into uint64 - exact whatever the launch geometry, no atomics.  No workgroup waits on another and no
// loop is longer than a dimension.
#include <type_traits>

#include "vu_common.h"
#include "../../include/vit_unet_amd.h"

namespace {

constexpr int RS_TX = 128, RS_TY = 8, RS_TZ = 1;   // the tile of one workgroup: 32 threads x 4 outputs along x, 8 rows, 1 slice
constexpr int RS_Q = 1 << 15;
static_assert(RS_TX / 4 * RS_TY * RS_TZ == 256 && RS_TX + RS_TY + RS_TZ <= 256, "one thread per quad, one thread per tap");

// the linear table rule of the header; n_in, n_out < 2^31 and i < n_out, so (2 i + 1) n_in < 2^63 and 2 Q r < 2^48
__host__ __device__ inline void rs_linear_tap(long long i, int n_in, int n_out, int* i0, int* w) {
  const long long num = (2 * i + 1) * (long long)n_in - n_out, den = 2LL * n_out;
  if (num <= 0) { *i0 = 0; *w = 0; return; }
  const long long q = num / den, r = num - q * den;
  if (q >= n_in - 1) { *i0 = n_in - 1; *w = 0; return; }
  *i0 = (int)q;
  *w = (int)((2LL * RS_Q * r + den) / (2 * den));
}

__host__ __device__ inline int rs_nearest_tap(long long i, int n_in, int n_out) {
  return (int)(((2 * i + 1) * (long long)n_in) / (2LL * n_out));
}

__device__ __forceinline__ int rs_stage(int a, int b, int w) { return (a * (RS_Q - w) + b * w + RS_Q / 2) >> 15; }
// subtraction, product and sum each rounded to float32 on its own.  hipcc contracts a * b + c into an fma by default, through
// __fmul_rn / __fadd_rn as well: the pragma takes the permission away from these three operations (the ISA has v_pk_add_f32 /
// v_pk_mul_f32 / v_pk_add_f32 per stage and no fma)
__device__ __forceinline__ float rs_stage(float a, float b, float wf) {
#pragma clang fp contract(off)
  const float d = b - a;
  const float t = d * wf;
  return a + t;
}

struct rs_dims { int Di, Hi, Wi, Do, Ho, Wo, nxb, nyb; };

__device__ __forceinline__ unsigned rs_wave_sum(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// T = int16_t: out only.  T = float: out / mask / partials, each may be null (the same in every thread of the launch).
// blockIdx.x = (z nyb + by) nxb + bx: the workgroups of one output slice are consecutive, as the counts kernel expects.
template <typename T>
__global__ __launch_bounds__(256) void resample_linear_kernel(const T* __restrict__ in, T* __restrict__ out, uint8_t* __restrict__ mask,
                                                              const uint8_t* __restrict__ truth, uint32_t* __restrict__ partials,
                                                              rs_dims d, float zthr, int label, int vec_out, int vec_mask,
                                                              int vec_truth) {
  constexpr bool F32 = sizeof(T) == 4;
  typedef typename std::conditional<F32, float, int>::type V;    // a value, and a weight, as a stage takes them
  __shared__ int sx0[RS_TX], sxw[RS_TX], sy0[RS_TY], syw[RS_TY], sz0[RS_TZ], szw[RS_TZ];
  __shared__ unsigned sm[2][4];
  const int t = threadIdx.x;
  const int bx = blockIdx.x % d.nxb, byz = blockIdx.x / d.nxb;
  const int by = byz % d.nyb, z = byz / d.nyb;
  if (t < RS_TX) {
    const int x = bx * RS_TX + t;
    int i0 = 0, w = 0;
    if (x < d.Wo) rs_linear_tap(x, d.Wi, d.Wo, &i0, &w);
    sx0[t] = i0; sxw[t] = w;
  } else if (t < RS_TX + RS_TY) {
    const int y = by * RS_TY + (t - RS_TX);
    int i0 = 0, w = 0;
    if (y < d.Ho) rs_linear_tap(y, d.Hi, d.Ho, &i0, &w);
    sy0[t - RS_TX] = i0; syw[t - RS_TX] = w;
  } else if (t < RS_TX + RS_TY + RS_TZ) {
    int i0, w;
    rs_linear_tap(z, d.Di, d.Do, &i0, &w);
    sz0[0] = i0; szw[0] = w;
  }
  __syncthreads();
  const int lx = (t & 31) * 4, ly = t >> 5;
  const int x0 = bx * RS_TX + lx, y = by * RS_TY + ly;
  unsigned c_pred = 0, c_true = 0, c_both = 0;
  if (y < d.Ho && x0 < d.Wo) {
    const int ya = sy0[ly], wy = syw[ly], za = sz0[0], wz = szw[0];
    const int yb = min(ya + 1, d.Hi - 1), zb = min(za + 1, d.Di - 1);
    // an integer stage with w = 0 returns its first tap exactly, so its second row is not read; the float stage always runs as written
    const bool two_y = F32 || wy != 0, two_z = F32 || wz != 0;
    const T* r00 = in + ((size_t)za * d.Hi + ya) * d.Wi;
    const T* r01 = in + ((size_t)za * d.Hi + yb) * d.Wi;
    const T* r10 = in + ((size_t)zb * d.Hi + ya) * d.Wi;
    const T* r11 = in + ((size_t)zb * d.Hi + yb) * d.Wi;
    V wyv, wzv;
    if constexpr (F32) { wyv = (float)wy * (1.0f / RS_Q); wzv = (float)wz * (1.0f / RS_Q); } else { wyv = wy; wzv = wz; }
    V v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[j] = 0;
      if (x0 + j < d.Wo) {
        const int xa = sx0[lx + j], wx = sxw[lx + j], xb = min(xa + 1, d.Wi - 1);
        V wxv;
        if constexpr (F32) wxv = (float)wx * (1.0f / RS_Q); else wxv = wx;
        const V a00 = rs_stage((V)r00[xa], (V)r00[xb], wxv);
        const V a01 = two_y ? rs_stage((V)r01[xa], (V)r01[xb], wxv) : a00;
        const V b0 = rs_stage(a00, a01, wyv);
        V b1 = b0;
        if (two_z) {
          const V a10 = rs_stage((V)r10[xa], (V)r10[xb], wxv);
          const V a11 = two_y ? rs_stage((V)r11[xa], (V)r11[xb], wxv) : a10;
          b1 = rs_stage(a10, a11, wyv);
        }
        v[j] = rs_stage(b0, b1, wzv);
      }
    }
    const size_t o = ((size_t)z * d.Ho + y) * d.Wo + x0;
    if (out) {
      if (vec_out) {           // Wo % 4 == 0 and an aligned buffer: the quad is whole and o % 4 == 0
        if constexpr (F32) {
          *reinterpret_cast<float4*>(out + o) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
          const s16x4 s = {(short)v[0], (short)v[1], (short)v[2], (short)v[3]};
          *reinterpret_cast<s16x4*>(out + o) = s;
        }
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (x0 + j < d.Wo) out[o + j] = (T)v[j];
      }
    }
    if constexpr (F32) {
      unsigned m[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) m[j] = (x0 + j < d.Wo && v[j] >= zthr) ? 1u : 0u;
      if (mask) {
        if (vec_mask) {
          *reinterpret_cast<uint32_t*>(mask + o) = m[0] | (m[1] << 8) | (m[2] << 16) | (m[3] << 24);
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (x0 + j < d.Wo) mask[o + j] = (uint8_t)m[j];
        }
      }
      if (partials) {
        unsigned tv[4] = {0u, 0u, 0u, 0u};
        if (vec_truth) {
          const uint32_t u = *reinterpret_cast<const uint32_t*>(truth + o);
          tv[0] = u & 255u; tv[1] = (u >> 8) & 255u; tv[2] = (u >> 16) & 255u; tv[3] = u >> 24;
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (x0 + j < d.Wo) tv[j] = truth[o + j];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const unsigned tj = (x0 + j < d.Wo && (label < 0 ? tv[j] != 0u : tv[j] == (unsigned)label)) ? 1u : 0u;
          c_pred += m[j]; c_true += tj; c_both += m[j] & tj;
        }
      }
    }
  }
  if constexpr (F32) {
    if (!partials) return;   // the same in every thread of the launch
    // a workgroup owns at most 1024 pixels: pred and both share one word (16 bits each)
    const unsigned a = rs_wave_sum(c_pred | (c_both << 16)), b = rs_wave_sum(c_true);
    const int wv = t >> 6;
    if ((t & 63) == 0) { sm[0][wv] = a; sm[1][wv] = b; }
    __syncthreads();
    if (t == 0) {
      const unsigned sa = sm[0][0] + sm[0][1] + sm[0][2] + sm[0][3], sb = sm[1][0] + sm[1][1] + sm[1][2] + sm[1][3];
      uint32_t* p = partials + (size_t)blockIdx.x * 3;
      p[0] = sa & 0xffffu; p[1] = sb; p[2] = sa >> 16;
    }
  }
}

// one block per output slice: thread i sums partials i, i + 256, ..., then a fixed tree over the 256 threads
__global__ __launch_bounds__(256) void resample_counts_kernel(const uint32_t* __restrict__ partials, unsigned long long* __restrict__ counts,
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

__global__ __launch_bounds__(256) void resample_nearest_u8_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, rs_dims d,
                                                                  int vec_out) {
  __shared__ int sx[RS_TX], sy[RS_TY], sz[RS_TZ];
  const int t = threadIdx.x;
  const int bx = blockIdx.x % d.nxb, byz = blockIdx.x / d.nxb;
  const int by = byz % d.nyb, z = byz / d.nyb;
  if (t < RS_TX) {
    const int x = bx * RS_TX + t;
    sx[t] = x < d.Wo ? rs_nearest_tap(x, d.Wi, d.Wo) : 0;
  } else if (t < RS_TX + RS_TY) {
    const int y = by * RS_TY + (t - RS_TX);
    sy[t - RS_TX] = y < d.Ho ? rs_nearest_tap(y, d.Hi, d.Ho) : 0;
  } else if (t < RS_TX + RS_TY + RS_TZ) {
    sz[0] = rs_nearest_tap(z, d.Di, d.Do);
  }
  __syncthreads();
  const int lx = (t & 31) * 4, ly = t >> 5;
  const int x0 = bx * RS_TX + lx, y = by * RS_TY + ly;
  if (y >= d.Ho || x0 >= d.Wo) return;
  const uint8_t* row = in + ((size_t)sz[0] * d.Hi + sy[ly]) * d.Wi;
  unsigned v[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = x0 + j < d.Wo ? row[sx[lx + j]] : 0u;
  const size_t o = ((size_t)z * d.Ho + y) * d.Wo + x0;
  if (vec_out) {
    *reinterpret_cast<uint32_t*>(out + o) = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (x0 + j < d.Wo) out[o + j] = (uint8_t)v[j];
  }
}

inline bool aligned_to(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

inline bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + nb && b0 < a0 + na;
}

// a b c <= 2^31 - 1 for positive ints, without leaving 64 bits on the way
inline bool fits_int(int a, int b, int c) {
  const long long p = (long long)a * b;
  return p <= 0x7fffffffLL && p * c <= 0x7fffffffLL;
}

// the shape checks every entry shares; fills the launch geometry.  elements <= 2^31 - 1 bounds the workgroup count as well
int check_shapes(const char* who, int Di, int Hi, int Wi, int Do, int Ho, int Wo, rs_dims* d) {
  VU_REQUIRE(Di >= 1 && Hi >= 1 && Wi >= 1 && Do >= 1 && Ho >= 1 && Wo >= 1, "%s: every dimension must be at least 1 (got %d x %d x %d -> %d x %d x %d)",
             who, Di, Hi, Wi, Do, Ho, Wo);
  VU_REQUIRE(fits_int(Di, Hi, Wi) && fits_int(Do, Ho, Wo),
             "%s: more than 2^31 - 1 elements (%d x %d x %d -> %d x %d x %d)", who, Di, Hi, Wi, Do, Ho, Wo);
  d->Di = Di; d->Hi = Hi; d->Wi = Wi; d->Do = Do; d->Ho = Ho; d->Wo = Wo;
  d->nxb = vu_cdiv(Wo, RS_TX); d->nyb = vu_cdiv(Ho, RS_TY);
  return VU_OK;
}

inline long long blocks_of(const rs_dims& d) { return (long long)d.nxb * d.nyb * d.Do; }   // <= Do Ho Wo <= 2^31 - 1

}  // namespace

extern "C" {

int vu_resample_axis_linear(int n_in, int n_out, int* i0, int* w, int capacity) {
  VU_REQUIRE(n_in >= 1 && n_out >= 1, "resample_axis_linear: lengths must be at least 1 (got %d -> %d)", n_in, n_out);
  VU_REQUIRE(i0 && w, "resample_axis_linear: null argument");
  VU_REQUIRE(capacity >= n_out, "resample_axis_linear: the tables hold %d entries, %d are needed", capacity, n_out);
  for (int i = 0; i < n_out; ++i) rs_linear_tap(i, n_in, n_out, &i0[i], &w[i]);
  return n_out;
}

int vu_resample_axis_nearest(int n_in, int n_out, int* src, int capacity) {
  VU_REQUIRE(n_in >= 1 && n_out >= 1, "resample_axis_nearest: lengths must be at least 1 (got %d -> %d)", n_in, n_out);
  VU_REQUIRE(src, "resample_axis_nearest: null argument");
  VU_REQUIRE(capacity >= n_out, "resample_axis_nearest: the table holds %d entries, %d are needed", capacity, n_out);
  for (int i = 0; i < n_out; ++i) src[i] = rs_nearest_tap(i, n_in, n_out);
  return n_out;
}

int vu_resample_geometry(int* tile_x, int* tile_y, int* tile_z) {
  VU_REQUIRE(tile_x && tile_y && tile_z, "resample_geometry: null argument");
  *tile_x = RS_TX; *tile_y = RS_TY; *tile_z = RS_TZ;
  return VU_OK;
}

int vu_resample_i16(const int16_t* in, int16_t* out, int Di, int Hi, int Wi, int Do, int Ho, int Wo, void* stream) {
  VU_REQUIRE(in && out, "resample_i16: null argument");
  rs_dims d;
  int rc = check_shapes("resample_i16", Di, Hi, Wi, Do, Ho, Wo, &d);
  if (rc) return rc;
  const size_t ni = (size_t)Di * Hi * Wi, no = (size_t)Do * Ho * Wo;
  VU_REQUIRE(!ranges_overlap(in, ni * 2, out, no * 2), "resample_i16: the output must not alias the input");
  const int vec_out = (Wo % 4 == 0 && aligned_to(out, 8)) ? 1 : 0;
  hipLaunchKernelGGL(resample_linear_kernel<int16_t>, dim3((unsigned)blocks_of(d)), dim3(256), 0, (hipStream_t)stream, in, out,
                     (uint8_t*)nullptr, (const uint8_t*)nullptr, (uint32_t*)nullptr, d, 0.f, -1, vec_out, 0, 0);
  if (vu_prof_on()) vu_prof_note("resample_i16_kernel", 0.0, 2.0 * ni + 2.0 * no);
  return vu_check_launch("vu_resample_i16");
}

int vu_resample_u8_nearest(const uint8_t* in, uint8_t* out, int Di, int Hi, int Wi, int Do, int Ho, int Wo, void* stream) {
  VU_REQUIRE(in && out, "resample_u8_nearest: null argument");
  rs_dims d;
  int rc = check_shapes("resample_u8_nearest", Di, Hi, Wi, Do, Ho, Wo, &d);
  if (rc) return rc;
  const size_t ni = (size_t)Di * Hi * Wi, no = (size_t)Do * Ho * Wo;
  VU_REQUIRE(!ranges_overlap(in, ni, out, no), "resample_u8_nearest: the output must not alias the input");
  const int vec_out = (Wo % 4 == 0 && aligned_to(out, 4)) ? 1 : 0;
  hipLaunchKernelGGL(resample_nearest_u8_kernel, dim3((unsigned)blocks_of(d)), dim3(256), 0, (hipStream_t)stream, in, out, d, vec_out);
  if (vu_prof_on()) vu_prof_note("resample_u8_nearest_kernel", 0.0, 1.0 * ni + 1.0 * no);
  return vu_check_launch("vu_resample_u8_nearest");
}

size_t vu_resample_f32_scratch_bytes(int Do, int Ho, int Wo) {
  if (Do <= 0 || Ho <= 0 || Wo <= 0) return 0;
  return (size_t)Do * (size_t)vu_cdiv(Wo, RS_TX) * (size_t)vu_cdiv(Ho, RS_TY) * 3 * sizeof(uint32_t);
}

int vu_resample_f32(const float* in, const uint8_t* truth, float* out, uint8_t* mask, unsigned long long* counts, void* scratch,
                    size_t scratch_bytes, int Di, int Hi, int Wi, int Do, int Ho, int Wo, float zthr, int label, void* stream) {
  VU_REQUIRE(in && (out || mask || counts), "resample_f32: null argument (the input, and at least one of out / mask / counts)");
  VU_REQUIRE(!counts || truth, "resample_f32: counts need a truth volume");
  rs_dims d;
  int rc = check_shapes("resample_f32", Di, Hi, Wi, Do, Ho, Wo, &d);
  if (rc) return rc;
  VU_REQUIRE(label <= 255, "resample_f32: label must be negative (any non-zero truth) or 0 .. 255 (got %d)", label);
  VU_REQUIRE(zthr == zthr, "resample_f32: the threshold is not a number");
  const size_t ni = (size_t)Di * Hi * Wi * 4, no = (size_t)Do * Ho * Wo;
  VU_REQUIRE(!(out && ranges_overlap(in, ni, out, no * 4)) && !(mask && ranges_overlap(in, ni, mask, no)) &&
                 !(counts && ranges_overlap(in, ni, counts, (size_t)Do * 24)),
             "resample_f32: the outputs must not alias the input");
  VU_REQUIRE(!(out && mask && ranges_overlap(out, no * 4, mask, no)) && !(counts && truth && mask && ranges_overlap(truth, no, mask, no)) &&
                 !(counts && truth && out && ranges_overlap(truth, no, out, no * 4)),
             "resample_f32: out, mask and truth must not overlap each other");
  if (counts) {
    const size_t need = vu_resample_f32_scratch_bytes(Do, Ho, Wo);
    VU_REQUIRE(scratch && scratch_bytes >= need && aligned_to(scratch, 4), "resample_f32: scratch too small or misaligned (%zu bytes needed)",
               need);
    VU_REQUIRE(aligned_to(counts, 8), "resample_f32: counts must be 8-byte aligned");
    VU_REQUIRE(!ranges_overlap(in, ni, scratch, need) && !ranges_overlap(truth, no, scratch, need) &&
                   !(out && ranges_overlap(out, no * 4, scratch, need)) && !(mask && ranges_overlap(mask, no, scratch, need)) &&
                   !ranges_overlap(counts, (size_t)Do * 24, scratch, need),
               "resample_f32: the scratch must not alias another buffer");
  }
  hipStream_t st = (hipStream_t)stream;
  const int w4 = Wo % 4 == 0;
  const int vec_out = (out && w4 && aligned_to(out, 16)) ? 1 : 0, vec_mask = (mask && w4 && aligned_to(mask, 4)) ? 1 : 0;
  const int vec_truth = (counts && w4 && aligned_to(truth, 4)) ? 1 : 0;
  hipLaunchKernelGGL(resample_linear_kernel<float>, dim3((unsigned)blocks_of(d)), dim3(256), 0, st, in, out, mask, truth,
                     counts ? (uint32_t*)scratch : (uint32_t*)nullptr, d, zthr, label, vec_out, vec_mask, vec_truth);
  if (vu_prof_on())
    vu_prof_note("resample_f32_kernel", 0.0, (double)ni + ((out ? 4.0 : 0.0) + (mask ? 1.0 : 0.0) + (counts ? 1.0 : 0.0)) * no);
  rc = vu_check_launch("vu_resample_f32");
  if (rc || !counts) return rc;
  hipLaunchKernelGGL(resample_counts_kernel, dim3(Do), dim3(256), 0, st, (const uint32_t*)scratch, counts, d.nxb * d.nyb);
  return vu_check_launch("vu_resample_f32/counts");
}

}  // extern "C"
