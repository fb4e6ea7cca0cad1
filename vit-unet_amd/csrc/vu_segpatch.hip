// Native-resolution segmentation training patches with foreground sampling: the int16 / label-mask twin of csrc/vu_patch.hip.
// A (D,H,W) int16 volume and its (D,H,W) uint8 label mask are cut into T x T crops of single slices, each under one of the
// eight dihedral ops of csrc/vu_patch.hip, and a chosen share of the crops is drawn ON THE DEVICE so that it holds a
// foreground pixel.  Three entries (include/vit_unet_amd.h has the formulas):
//   vu_fg_index          index[r] = foreground pixels in rows [0, r) of the volume taken as D H rows (index[D H] = total)
//   vu_segpatch_draw     (n,4) random words -> (n,4) crops (z, y0, x0, op): the r-th foreground pixel in raster order (found
//                        through the index) plus an offset inside the patch, or a uniform origin
//   vu_patch_pairs_i16   x = D_op(window(vol crop)), y = D_op(smoothed label of the mask crop), (n,1,T,T) float32 each
// A foreground pixel is mask != 0 (label < 0) or mask == label: the rule of vu_seg_blend (csrc/vu_segtile.hip).
//
// Index.  Pass 1: one wave per row, lanes stride over the row (one 4-byte load = 4 mask bytes where W % 4 == 0 and the
// buffer is 4-byte aligned, byte loads otherwise), a shuffle sum, one count per row into `scratch`.  Pass 2 and 3 are an
// exclusive scan with a FIXED geometry of 256 blocks x 256 threads whatever the size: block b owns the rows [b C, (b+1) C),
// C = ceil(D H / 256); pass 2 writes the 256 chunk totals, pass 3 adds the totals of the chunks before its own and scans its
// chunk 256 rows at a time.  Integers, no atomics: the same bits on every run.
// Draw.  One wave per crop.  The row of the r-th pixel is found by a 64-ary search of the index - every lane probes its own
// position, so the loop's loads are vector loads of lane-dependent addresses, not wave-uniform loads inside a loop (DESIGN
// 2a) - and the pixel inside the row by ballots over 64 pixels at a time.  The words the wave shares (the random words, the
// total) are read once, before any loop.  The search and the walk are bounded whatever index and mask hold.
// Cut.  patch_pairs_kernel's structure: a block owns one 32 x 32 tile of one crop, one thread = 4 consecutive output columns,
// transposing ops staged through a padded [32][33] LDS tile in which the int16 value and the label byte of a pixel share one
// dword, 16-byte stores where T % 4 == 0 and the buffer is aligned.  The crop entry is read once per block, before any loop,
// and clamped: no table content makes the kernel read outside the volume.
#include "vu_common.h"
#include "vu_data.h"
#include "../../include/vit_unet_amd.h"

namespace {

constexpr int TS = 32;          // tile side of the cut; 256 threads = 32 rows x 8 quads
constexpr int SCAN_BLOCKS = 256;   // fixed geometry of the scan: 256 blocks of 256 threads

__device__ __forceinline__ unsigned is_fg(unsigned m, int label) { return (label < 0 ? m != 0u : m == (unsigned)label) ? 1u : 0u; }

__device__ __forceinline__ unsigned wave_sum_u32(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// block sum over 256 threads; result valid in all threads.  `sm` holds 4 words.
__device__ __forceinline__ unsigned block_sum_u32(unsigned v, unsigned* sm) {
  v = wave_sum_u32(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
  __syncthreads();
  return sm[0] + sm[1] + sm[2] + sm[3];
}

// ---------------------------------------------------------------- index
// one wave per row: 4 rows per block
__global__ __launch_bounds__(256) void fg_rows_kernel(const uint8_t* __restrict__ mask, uint32_t* __restrict__ counts, int R, int W,
                                                      int label, int vec) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= R) return;   // the whole wave
  const uint8_t* p = mask + (size_t)row * W;
  unsigned c = 0;
  if (vec) {
    const uint32_t* p4 = reinterpret_cast<const uint32_t*>(p);
    for (int q = lane; q < (W >> 2); q += 64) {
      const uint32_t u = p4[q];
      c += is_fg(u & 255u, label) + is_fg((u >> 8) & 255u, label) + is_fg((u >> 16) & 255u, label) + is_fg(u >> 24, label);
    }
  } else {
    for (int x = lane; x < W; x += 64) c += is_fg(p[x], label);
  }
  c = wave_sum_u32(c);
  if (lane == 0) counts[row] = c;
}

// block b: total of the row counts of its chunk [b C, min((b+1) C, R))
__global__ __launch_bounds__(256) void fg_chunk_kernel(const uint32_t* __restrict__ counts, uint32_t* __restrict__ sums, int R, int C) {
  __shared__ unsigned sm[4];
  const long long lo = (long long)blockIdx.x * C, hi = min(lo + C, (long long)R);
  unsigned c = 0;
  for (long long r = lo + threadIdx.x; r < hi; r += 256) c += counts[r];
  c = block_sum_u32(c, sm);
  if (threadIdx.x == 0) sums[blockIdx.x] = c;
}

// block b: index[r + 1] = counts[0] + ... + counts[r] for the rows of its chunk; block 0 also writes index[0] = 0
__global__ __launch_bounds__(256) void fg_scan_kernel(const uint32_t* __restrict__ counts, const uint32_t* __restrict__ sums,
                                                      uint32_t* __restrict__ index, int R, int C) {
  __shared__ unsigned sm[4], wt[4];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  unsigned run = block_sum_u32(t < (int)blockIdx.x ? sums[t] : 0u, sm);   // rows before this chunk (256 chunks = 256 threads)
  if (blockIdx.x == 0 && t == 0) index[0] = 0u;
  const long long lo = (long long)blockIdx.x * C, hi = min(lo + C, (long long)R);
  for (long long base = lo; base < hi; base += 256) {
    const long long r = base + t;
    unsigned v = r < hi ? counts[r] : 0u;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned u = __shfl_up(v, o, 64);
      if (lane >= o) v += u;
    }
    __syncthreads();   // wt of the previous round has been read
    if (lane == 63) wt[wv] = v;
    __syncthreads();
    unsigned before = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k)
      if (k < wv) before += wt[k];
    if (r < hi) index[r + 1] = run + before + v;
    run += wt[0] + wt[1] + wt[2] + wt[3];
  }
}

// ---------------------------------------------------------------- draw
// one wave (one block of 64 threads) per crop
__global__ __launch_bounds__(64) void segpatch_draw_kernel(const uint8_t* __restrict__ mask, const uint32_t* __restrict__ index,
                                                           const uint32_t* __restrict__ rnd, int* __restrict__ crops, int D, int H,
                                                           int W, int T, uint32_t fg_thresh, int label) {
  const int i = blockIdx.x, lane = threadIdx.x;
  const int R = D * H;
  // shared by the wave: read once, before any loop
  const uint4 w = *reinterpret_cast<const uint4*>(rnd + (size_t)4 * i);
  const uint32_t total = index[R];
  const uint32_t hy = w.z >> 16, hx = w.z & 0xffffu;
  int z, y0, x0;
  if (w.x < fg_thresh && total > 0u) {
    const uint32_t r = (uint32_t)(((unsigned long long)w.y * total) >> 32);
    // 64-ary search for the row: index[lo] <= r < index[hi]; lane l probes lo + (l + 1) step.  Ends in at most 6 rounds
    // (the span shrinks to at most ceil(span / 64) a round) whatever the index holds, with lo in [0, R - 1].
    int lo = 0, hi = R;
    while (hi - lo > 1) {
      const int span = hi - lo, step = (span + 63) >> 6;
      const long long probe = (long long)lo + (long long)(lane + 1) * step;
      const int p = (int)(probe < hi ? probe : hi);
      const bool ok = p < hi && index[p] <= r;
      const int c = __popcll(__ballot(ok));   // a prefix of the lanes for a monotonic index
      const long long nlo = (long long)lo + (long long)c * step, nhi = nlo + step;
      hi = (int)(nhi < hi ? nhi : hi);
      lo = (int)(nlo < hi - 1 ? nlo : hi - 1);
    }
    // walk the row: the k-th foreground pixel of it, 64 pixels a round; stays at W - 1 when the row holds fewer
    uint32_t k = r - index[lo];
    const uint8_t* row = mask + (size_t)lo * W;
    int x = W - 1;
    for (int xb = 0; xb < W; xb += 64) {
      const bool f = xb + lane < W && is_fg(row[xb + lane], label) != 0u;
      unsigned long long b = __ballot(f);
      const uint32_t c = (uint32_t)__popcll(b);
      if (k < c) {
        for (uint32_t q = 0; q < k; ++q) b &= b - 1ull;   // drop the k lowest set bits
        x = xb + __ffsll((long long)b) - 1;
        break;
      }
      k -= c;
    }
    const int y = lo % H;
    z = lo / H;
    const int oy = (int)((hy * (uint32_t)T) >> 16), ox = (int)((hx * (uint32_t)T) >> 16);
    y0 = min(max(y - oy, 0), H - T);
    x0 = min(max(x - ox, 0), W - T);
  } else {
    z = (int)(((unsigned long long)w.y * (unsigned)D) >> 32);
    y0 = (int)((hy * (uint32_t)(H - T + 1)) >> 16);
    x0 = (int)((hx * (uint32_t)(W - T + 1)) >> 16);
  }
  if (lane == 0) *reinterpret_cast<int4*>(crops + (size_t)4 * i) = make_int4(z, y0, x0, (int)(w.w & 7u));
}

// ---------------------------------------------------------------- cut
struct dihedral_map {
  int tr, fy, fx;
};

__device__ __forceinline__ dihedral_map make_map(int op) {   // csrc/vu_patch.hip
  const int k = op & 3;
  dihedral_map m;
  m.tr = k & 1;
  m.fy = k >> 1;
  m.fx = ((k ^ (k >> 1)) & 1) ^ ((op >> 2) & 1);
  return m;
}

__device__ __forceinline__ int flip_if(int f, int T, int v) { return f ? T - 1 - v : v; }

// int16 value in the low half, label byte above it
__device__ __forceinline__ uint32_t load_px(const int16_t* __restrict__ vol, const uint8_t* __restrict__ mask, size_t off) {
  uint32_t w = 0;
  if (vol) w = (uint32_t)(uint16_t)vol[off];
  if (mask) w |= (uint32_t)mask[off] << 16;
  return w;
}

// one block = one 32 x 32 tile of one crop, slice and mask.  The op is per crop (table in device memory), so the choice
// between the direct and the transposing form is a branch that is uniform over the block.
__global__ __launch_bounds__(256) void patch_pairs_i16_kernel(const int16_t* __restrict__ vol, const uint8_t* __restrict__ mask,
                                                              float* __restrict__ x, float* __restrict__ y, int D, int H, int W, int T,
                                                              int nt, const int* __restrict__ crops, float lo, float range, float keep,
                                                              float floor_, int label, int vecx, int vecy) {
  __shared__ uint32_t lds[TS][TS + 1];
  const int per = nt * nt;
  const int crop = blockIdx.x / per, tile = blockIdx.x % per;
  const int i0 = (tile / nt) * TS, j0 = (tile % nt) * TS;
  // the table is device data the host never saw: read once, clamp, so that no content can make the kernel read outside the volume
  const int4 ct = *reinterpret_cast<const int4*>(crops + (size_t)4 * crop);
  const int z = min(max(ct.x, 0), D - 1), y0 = min(max(ct.y, 0), H - T), x0 = min(max(ct.z, 0), W - T);
  const dihedral_map m = make_map(ct.w & 7);
  const size_t slice = (size_t)z * H * W;
  const int r = threadIdx.x >> 3, q4 = (threadIdx.x & 7) * 4;
  uint32_t px[4] = {0u, 0u, 0u, 0u};
  if (m.tr) {
    // fill along source rows: lane c of a 32-lane half = source column of output row i0 + c, 4 passes of 8 source rows
    const int c = threadIdx.x & 31, i = i0 + c;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int rr = (threadIdx.x >> 5) + 8 * k, j = j0 + rr;
      if (i < T && j < T) lds[rr][c] = load_px(vol, mask, slice + (size_t)(y0 + flip_if(m.fy, T, j)) * W + x0 + flip_if(m.fx, T, i));
    }
    __syncthreads();
  }
  const int i = i0 + r, j = j0 + q4;
  if (i >= T || j >= T) return;
  if (m.tr) {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (j + e < T) px[e] = lds[q4 + e][r];
  } else {
    const size_t row = slice + (size_t)(y0 + flip_if(m.fy, T, i)) * W + x0;
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (j + e < T) px[e] = load_px(vol, mask, row + flip_if(m.fx, T, j + e));
  }
  const size_t base = (size_t)crop * T * T + (size_t)i * T + j;
  if (vol) {
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = vu_window_i16((int)(int16_t)(px[e] & 0xffffu), lo, range);
    float* o = x + base;
    if (vecx) {
      *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (j + e < T) o[e] = v[e];
    }
  }
  if (mask) {
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = __fadd_rn(__fmul_rn((float)is_fg((px[e] >> 16) & 255u, label), keep), floor_);   // warp_seg_kernel
    float* o = y + base;
    if (vecy) {
      *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (j + e < T) o[e] = v[e];
    }
  }
}

inline bool aligned_to(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

inline int check_volume(const char* who, int D, int H, int W, int label) {
  VU_REQUIRE(D >= 1 && H >= 1 && W >= 1, "%s: empty volume (%d x %d x %d)", who, D, H, W);
  VU_REQUIRE((unsigned long long)D * (unsigned long long)H * (unsigned long long)W < (1ull << 32) &&
                 (long long)D * H < 0x7fffffffLL,
             "%s: a volume of %d x %d x %d is too large (D H W must stay below 2^32 pixels)", who, D, H, W);
  VU_REQUIRE(label <= 255, "%s: label must be negative (any non-zero mask value) or 0 .. 255 (got %d)", who, label);
  return VU_OK;
}

}  // namespace

extern "C" {

size_t vu_fg_index_bytes(int D, int H) {
  if (D <= 0 || H <= 0) return 0;
  return ((size_t)D * (size_t)H + SCAN_BLOCKS) * sizeof(uint32_t);
}

int vu_fg_index(const uint8_t* mask, uint32_t* index, void* scratch, size_t scratch_bytes, int D, int H, int W, int label,
                void* stream) {
  int rc = check_volume("fg_index", D, H, W, label);
  if (rc) return rc;
  VU_REQUIRE(mask && index && scratch, "fg_index: null argument");
  const size_t need = vu_fg_index_bytes(D, H);
  VU_REQUIRE(scratch_bytes >= need && aligned_to(scratch, 4), "fg_index: scratch too small or misaligned (%zu bytes needed)", need);
  VU_REQUIRE(aligned_to(index, 4), "fg_index: the index must be 4-byte aligned");
  const int R = D * H, C = vu_cdiv(R, SCAN_BLOCKS);
  uint32_t* counts = (uint32_t*)scratch;
  uint32_t* sums = counts + R;
  hipStream_t st = (hipStream_t)stream;
  const int vec = (W % 4 == 0 && aligned_to(mask, 4)) ? 1 : 0;
  hipLaunchKernelGGL(fg_rows_kernel, dim3((unsigned)vu_cdiv(R, 4)), dim3(256), 0, st, mask, counts, R, W, label, vec);
  if (vu_prof_on()) vu_prof_note("fg_rows_kernel", 0.0, (double)R * W + 4.0 * R);
  rc = vu_check_launch("vu_fg_index/rows");
  if (rc) return rc;
  hipLaunchKernelGGL(fg_chunk_kernel, dim3(SCAN_BLOCKS), dim3(256), 0, st, (const uint32_t*)counts, sums, R, C);
  rc = vu_check_launch("vu_fg_index/chunks");
  if (rc) return rc;
  hipLaunchKernelGGL(fg_scan_kernel, dim3(SCAN_BLOCKS), dim3(256), 0, st, (const uint32_t*)counts, (const uint32_t*)sums, index, R, C);
  if (vu_prof_on()) vu_prof_note("fg_scan_kernel", 0.0, 8.0 * R);
  return vu_check_launch("vu_fg_index");
}

int vu_segpatch_draw(const uint8_t* mask, const uint32_t* index, const uint32_t* rnd, int* crops, int n, int D, int H, int W, int T,
                     uint32_t fg_thresh, int label, void* stream) {
  int rc = check_volume("segpatch_draw", D, H, W, label);
  if (rc) return rc;
  VU_REQUIRE(T >= 1, "segpatch_draw: the patch size must be positive (got %d)", T);
  VU_REQUIRE(H >= T && W >= T, "segpatch_draw: a %d x %d slice is smaller than a patch of %d", H, W, T);
  VU_REQUIRE(H <= 65535 && W <= 65535, "segpatch_draw: a %d x %d slice is too large (65535 a side: 16-bit offsets)", H, W);
  VU_REQUIRE(n >= 1, "segpatch_draw: no crop (n = %d)", n);
  VU_REQUIRE(mask && index && rnd && crops, "segpatch_draw: null argument");
  VU_REQUIRE(aligned_to(rnd, 16) && aligned_to(crops, 16) && aligned_to(index, 4),
             "segpatch_draw: the random words and the crop table must be 16-byte aligned, the index 4-byte aligned");
  hipLaunchKernelGGL(segpatch_draw_kernel, dim3((unsigned)n), dim3(64), 0, (hipStream_t)stream, mask, index, rnd, crops, D, H, W, T,
                     fg_thresh, label);
  if (vu_prof_on()) vu_prof_note("segpatch_draw_kernel", 0.0, 32.0 * n);
  return vu_check_launch("vu_segpatch_draw");
}

int vu_patch_pairs_i16(const int16_t* vol, const uint8_t* mask, float* x, float* y, int D, int H, int W, int T, const int* crops, int n,
                       float lo, float hi, float ls, int label, void* stream) {
  int rc = check_volume("patch_pairs_i16", D, H, W, label);
  if (rc) return rc;
  VU_REQUIRE(T >= 1, "patch_pairs_i16: the patch size must be positive (got %d)", T);
  VU_REQUIRE(H >= T && W >= T, "patch_pairs_i16: a %d x %d slice is smaller than a patch of %d (small slices are refused, not reflected)",
             H, W, T);
  VU_REQUIRE(n >= 1, "patch_pairs_i16: no crop (n = %d)", n);
  VU_REQUIRE(hi > lo, "patch_pairs_i16: intensity window must have hi > lo (got %g..%g)", (double)lo, (double)hi);
  VU_REQUIRE(ls >= 0.f && ls < 1.f, "patch_pairs_i16: label smoothing must be in [0,1) (got %g)", (double)ls);
  VU_REQUIRE((vol && x) || (mask && y), "patch_pairs_i16: null argument: nothing to do (no vol/x and no mask/y pair)");
  VU_REQUIRE((vol == nullptr) == (x == nullptr) && (mask == nullptr) == (y == nullptr),
             "patch_pairs_i16: null argument: input and output of a pair must both be given");
  VU_REQUIRE(crops, "patch_pairs_i16: null argument (the crop table)");
  VU_REQUIRE(aligned_to(crops, 16) && (!vol || aligned_to(vol, 2)), "patch_pairs_i16: the crop table must be 16-byte aligned, the volume 2-byte aligned");
  const int nt = vu_cdiv(T, TS);
  const long long blocks = (long long)n * nt * nt;
  VU_REQUIRE(blocks <= 0x7fffffffLL, "patch_pairs_i16: launch too large (%d crops of %d)", n, T);
  const int vecx = (x && T % 4 == 0 && aligned_to(x, 16)) ? 1 : 0, vecy = (y && T % 4 == 0 && aligned_to(y, 16)) ? 1 : 0;
  hipLaunchKernelGGL(patch_pairs_i16_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, vol, mask, x, y, D, H, W, T, nt,
                     crops, lo, hi - lo, 1.0f - ls, 0.5f * ls, label, vecx, vecy);
  if (vu_prof_on()) vu_prof_note("patch_pairs_i16_kernel", 0.0, (double)n * T * T * ((vol ? 6.0 : 0.0) + (mask ? 5.0 : 0.0)) + 16.0 * n);
  return vu_check_launch("vu_patch_pairs_i16");
}

}  // extern "C"
