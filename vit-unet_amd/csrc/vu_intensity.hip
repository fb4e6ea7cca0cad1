// Per-volume intensity statistics: the exact 65536-bin histogram of an int16 volume under a voxel selection, the bounding box of the
// selected voxels, and from the histogram the count, extremes, power sums and order statistics that a per-volume intensity window is
// made of (Python: segment.IntensityNormalizer).  Integers only - no float arithmetic anywhere - and integer atomics, whose result does
// not depend on order (the precedent is vu_segclean.hip), so every output is the same bits on every run.  The contract is in
// include/vit_unet_amd.h.
//
// vu_intensity_hist is the only pass over the volume.  Two launches:
//   (a) intensity_clear_kernel   zeroes hist and sets bbox to the empty box (D, -1, H, -1, W, -1).
//   (b) intensity_hist_kernel    persistent workgroups of IH_THREADS threads, at most one per CU, stride over chunks of IH_V voxels.  A
//       lane loads 16 bytes = 8 voxels (with select 2 also 8 mask bytes) where the pointers allow, else 8 scalars IH_THREADS apart.  The
//       values IH_LDS_BASE .. IH_LDS_BASE + IH_LDS_BINS - 1 are counted in a private LDS sub-histogram (128 KiB: one workgroup per CU),
//       everything else goes straight to global atomics; at the end a workgroup adds its non-zero LDS bins to hist, 256 contiguous bytes
//       per wave-instruction.  The bounding box rides along: a thread keeps six extremes of its selected voxels (coordinates by two
//       divisions per 16-byte load and a carry per voxel), waves reduce them with shuffles, and six atomics per workgroup reach bbox.
//       Every lane of a wave runs every slot: the loop over chunks and slots is workgroup-uniform, validity is a flag.
//   Measurement forms (tools/build_variant.sh; numbers in DESIGN.md 4.19):
//   -DVU_INTENSITY_PEEL   a medical volume keeps a third to a half of its voxels in one bin (air) and same-address atomics serialise, so
//       a wave first peels wave-uniform values: round 0 ballots the lanes that hold the value that paid best so far (`hot`, a
//       wave-uniform register; no atomic at all when no lane holds it), round 1 broadcasts the first remaining lane's value and ballots
//       again; each round is ONE add of the population count by one lane, then what is left does its own atomic.  Measured on an
//       MI355X it halves the time of a constant volume and costs a quarter more on a CT-like one, where the LDS unit copes with the
//       air bin on its own: it is not in the product.
//   -DVU_INTENSITY_DIRECT   no LDS sub-histogram: every count is a global atomic (two orders of magnitude slower on a CT-like volume).
//   vu_intensity_geometry reports the LDS range that was built.
//
// vu_intensity_stats is one workgroup of 1024 threads over the histogram: a thread owns 64 consecutive bins, the counts are scanned
// across the workgroup in LDS, and the thread whose bins hold a wanted rank walks them.  N is read on the device.
#include "vu_common.h"
#include "../../include/vit_unet_amd.h"

namespace {

constexpr int IH_BINS = 65536, IH_OFFSET = 32768;   // hist[b] counts the value b - IH_OFFSET
constexpr int IH_THREADS = 1024, IH_PER_LANE = 8, IH_WAVES = IH_THREADS / 64;
constexpr int IH_V = IH_THREADS * IH_PER_LANE;      // voxels of one chunk
#ifdef VU_INTENSITY_DIRECT
constexpr int IH_LDS_BASE = 0, IH_LDS_BINS = 0;
#else
// CT (-1024 .. 3071 and its shifted variants) and 12 - 14 bit MR lie inside; 128 KiB leave room for the reduction scratch below
constexpr int IH_LDS_BASE = -16384, IH_LDS_BINS = 32768;
#endif
#ifdef VU_INTENSITY_PEEL
constexpr bool IH_PEEL = true;
#else
constexpr bool IH_PEEL = false;
#endif
constexpr size_t IH_LDS_BYTES = (size_t)IH_LDS_BINS * 4 + (size_t)IH_WAVES * 6 * 4;
static_assert(IH_LDS_BYTES <= 160 * 1024 && IH_LDS_BASE >= -IH_OFFSET && IH_LDS_BASE + IH_LDS_BINS <= IH_OFFSET, "LDS range");
static_assert(IH_BINS % IH_THREADS == 0 && IH_LDS_BINS % IH_THREADS == 0, "whole rounds of the workgroup");

struct ih_args {
  const int16_t* vol;
  const uint8_t* mask;
  uint32_t* hist;
  int32_t* bbox;
  uint32_t n, nchunks;   // voxels (< 2^32), chunks of IH_V
  int H, W, select, floor, label, vec;
};

__global__ __launch_bounds__(IH_THREADS) void intensity_clear_kernel(uint32_t* __restrict__ hist, int32_t* __restrict__ bbox, int D, int H,
                                                                      int W) {
  hist[blockIdx.x * IH_THREADS + threadIdx.x] = 0u;   // the grid is IH_BINS / IH_THREADS workgroups
  if (bbox && blockIdx.x == 0 && threadIdx.x < 6) {
    const int t = threadIdx.x;
    bbox[t] = (t & 1) ? -1 : (t == 0 ? D : t == 2 ? H : W);
  }
}

__device__ __forceinline__ void ih_add(uint32_t* lh, uint32_t* gh, int v, uint32_t c) {
  const uint32_t rel = (uint32_t)(v - IH_LDS_BASE);
  if (rel < (uint32_t)IH_LDS_BINS) atomicAdd(&lh[rel], c);
  else atomicAdd(&gh[v + IH_OFFSET], c);
}

// one slot of a wave: 64 values, `sel` says which count.  Called by all 64 lanes together.
__device__ __forceinline__ void ih_count(uint32_t* lh, uint32_t* gh, int v, bool sel, int& hot, int lane) {
  if (IH_PEEL) {
    unsigned long long pend = __ballot(sel);
    if (pend) {
      const unsigned long long m0 = __ballot(sel && v == hot);
      const uint32_t c0 = (uint32_t)__popcll(m0);
      if (c0) {
        if (lane == __ffsll((long long)m0) - 1) ih_add(lh, gh, hot, c0);
        pend &= ~m0;
      }
      if (pend) {
        const int leader = __builtin_amdgcn_readfirstlane(__ffsll((long long)pend) - 1);
        const int c = __builtin_amdgcn_readlane(v, leader);   // != hot: the leader is not in m0
        const unsigned long long m1 = __ballot(sel && v == c);
        const uint32_t c1 = (uint32_t)__popcll(m1);
        if (lane == leader) ih_add(lh, gh, c, c1);
        pend &= ~m1;
        if (c1 > c0) hot = c;
      }
      sel = (pend >> lane) & 1ull;
    }
  }
  if (sel) ih_add(lh, gh, v, 1u);
}

__device__ __forceinline__ bool ih_selected(int v, unsigned m, int select, int floor, int label) {
  return select == 0 ? true : select == 1 ? v > floor : (label < 0 ? m != 0u : m == (unsigned)label);
}

struct ih_box { int z0, z1, y0, y1, x0, x1; };
__device__ __forceinline__ void ih_box_add(ih_box& b, int z, int y, int x) {
  b.z0 = min(b.z0, z); b.z1 = max(b.z1, z); b.y0 = min(b.y0, y); b.y1 = max(b.y1, y); b.x0 = min(b.x0, x); b.x1 = max(b.x1, x);
}

__global__ __launch_bounds__(IH_THREADS) void intensity_hist_kernel(ih_args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  uint32_t* lh = reinterpret_cast<uint32_t*>(smem_raw);               // IH_LDS_BINS counters
  int* sbox = reinterpret_cast<int*>(smem_raw) + IH_LDS_BINS;          // IH_WAVES x 6
  const int t = threadIdx.x, lane = t & 63;
  for (int b = t; b < IH_LDS_BINS; b += IH_THREADS) lh[b] = 0u;
  __syncthreads();
  const bool want_box = a.bbox != nullptr;
  const uint32_t W = (uint32_t)a.W, H = (uint32_t)a.H;
  ih_box box = {0x7fffffff, -1, 0x7fffffff, -1, 0x7fffffff, -1};
  int hot = IH_OFFSET;   // no int16 value: the first round 1 sets it
  for (uint32_t c = blockIdx.x; c < a.nchunks; c += gridDim.x) {
    const uint32_t c0 = c * (uint32_t)IH_V;                            // < 2^32: c0 < n
    int v[IH_PER_LANE];
    bool s[IH_PER_LANE];
    const uint32_t i0 = c0 + (uint32_t)t * IH_PER_LANE;
    if (a.vec && a.n - c0 >= (uint32_t)IH_V) {
      // a whole chunk through 16-byte loads: the lane owns 8 consecutive voxels
      const uint4 q = *reinterpret_cast<const uint4*>(a.vol + i0);
      const uint32_t w[4] = {q.x, q.y, q.z, q.w};
      uint2 mq = make_uint2(0u, 0u);
      if (a.select == 2) mq = *reinterpret_cast<const uint2*>(a.mask + i0);
#pragma unroll
      for (int j = 0; j < IH_PER_LANE; ++j) {
        v[j] = (int)(int16_t)(uint16_t)(w[j >> 1] >> ((j & 1) * 16));
        const unsigned m = ((j < 4 ? mq.x : mq.y) >> ((j & 3) * 8)) & 255u;
        s[j] = ih_selected(v[j], m, a.select, a.floor, a.label);
      }
      if (want_box) {
        const uint32_t row = i0 / W;
        int x = (int)(i0 - row * W), z = (int)(row / H), y = (int)(row - (uint32_t)z * H);
#pragma unroll
        for (int j = 0; j < IH_PER_LANE; ++j) {
          if (s[j]) ih_box_add(box, z, y, x);
          if (++x == (int)W) { x = 0; if (++y == (int)H) { y = 0; ++z; } }
        }
      }
    } else {
      // unaligned pointers, or the last partial chunk: guarded scalar loads, consecutive lanes on consecutive voxels
#pragma unroll
      for (int j = 0; j < IH_PER_LANE; ++j) {
        const uint32_t off = (uint32_t)j * IH_THREADS + (uint32_t)t;   // < IH_V
        const bool in = off < a.n - c0;
        const uint32_t i = c0 + off;
        v[j] = 0;
        s[j] = false;
        if (in) {
          v[j] = (int)a.vol[i];
          const unsigned m = a.select == 2 ? (unsigned)a.mask[i] : 0u;
          s[j] = ih_selected(v[j], m, a.select, a.floor, a.label);
          if (want_box && s[j]) {
            const uint32_t row = i / W, z = row / H;
            ih_box_add(box, (int)z, (int)(row - z * H), (int)(i - row * W));
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < IH_PER_LANE; ++j) ih_count(lh, a.hist, v[j], s[j], hot, lane);
  }
  if (want_box) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      box.z0 = min(box.z0, __shfl_xor(box.z0, o, 64)); box.z1 = max(box.z1, __shfl_xor(box.z1, o, 64));
      box.y0 = min(box.y0, __shfl_xor(box.y0, o, 64)); box.y1 = max(box.y1, __shfl_xor(box.y1, o, 64));
      box.x0 = min(box.x0, __shfl_xor(box.x0, o, 64)); box.x1 = max(box.x1, __shfl_xor(box.x1, o, 64));
    }
    if (lane == 0) {
      int* p = sbox + (t >> 6) * 6;
      p[0] = box.z0; p[1] = box.z1; p[2] = box.y0; p[3] = box.y1; p[4] = box.x0; p[5] = box.x1;
    }
  }
  __syncthreads();   // every count of the workgroup is in lh (or already in hist), every wave's box in sbox
  if (want_box && t < 6) {
    int r = sbox[t];
    for (int w = 1; w < IH_WAVES; ++w) r = (t & 1) ? max(r, sbox[w * 6 + t]) : min(r, sbox[w * 6 + t]);
    // an empty workgroup holds (INT_MAX, -1, ...): it changes nothing
    if (t & 1) { if (r >= 0) atomicMax(&a.bbox[t], r); }
    else if (r != 0x7fffffff) atomicMin(&a.bbox[t], r);
  }
  for (int b = t; b < IH_LDS_BINS; b += IH_THREADS) {
    const uint32_t cnt = lh[b];
    if (cnt) atomicAdd(&a.hist[b + IH_LDS_BASE + IH_OFFSET], cnt);
  }
}

struct ih_quantiles { unsigned pn[4], pd[4]; int nq; };

// host and device: the rank arithmetic of the header.  (N - 1) pn < 2^32 * 10^6 < 2^52
__host__ __device__ inline void ih_rank(unsigned long long N, unsigned pn, unsigned pd, unsigned long long* k, unsigned* r) {
  const unsigned long long p = (N - 1) * pn;
  *k = p / pd;
  *r = (unsigned)(p - *k * pd);
}

__global__ __launch_bounds__(1024) void intensity_stats_kernel(const uint32_t* __restrict__ hist, long long* __restrict__ stats,
                                                               ih_quantiles q, int vec) {
  constexpr int PER = IH_BINS / 1024;   // 64 consecutive bins per thread
  __shared__ unsigned long long s_cnt[1024], s_sq[1024], s_target[8];
  __shared__ long long s_sum[1024];
  __shared__ int s_min[1024], s_max[1024];
  const int t = threadIdx.x, base = t * PER;
  unsigned long long cnt = 0, sq = 0;
  long long sum = 0;
  int mn = 0x7fffffff, mx = -0x7fffffff;
  auto take = [&](int b, uint32_t c) {
    if (c) {
      const int v = b - IH_OFFSET;
      cnt += c; sum += (long long)v * (long long)c; sq += (unsigned long long)(v * v) * c;
      mn = min(mn, v); mx = max(mx, v);
    }
  };
  if (vec) {
#pragma unroll 4
    for (int i = 0; i < PER; i += 4) {
      const uint4 c = *reinterpret_cast<const uint4*>(hist + base + i);
      take(base + i, c.x); take(base + i + 1, c.y); take(base + i + 2, c.z); take(base + i + 3, c.w);
    }
  } else {
#pragma unroll 8
    for (int i = 0; i < PER; ++i) take(base + i, hist[base + i]);
  }
  s_cnt[t] = cnt; s_sq[t] = sq; s_sum[t] = sum; s_min[t] = mn; s_max[t] = mx;
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) {      // sums and extremes: a fixed tree
    if (t < o) { s_sq[t] += s_sq[t + o]; s_sum[t] += s_sum[t + o]; s_min[t] = min(s_min[t], s_min[t + o]); s_max[t] = max(s_max[t], s_max[t + o]); }
    __syncthreads();
  }
  for (int o = 1; o < 1024; o <<= 1) {     // inclusive scan of the counts
    const unsigned long long add = t >= o ? s_cnt[t - o] : 0ull;
    __syncthreads();
    s_cnt[t] += add;
    __syncthreads();
  }
  const unsigned long long incl = s_cnt[t], excl = incl - cnt, N = s_cnt[1023];
  if (t == 0) {
    stats[0] = (long long)N;
    stats[1] = N ? s_min[0] : 0; stats[2] = N ? s_max[0] : 0; stats[3] = N ? s_sum[0] : 0; stats[4] = N ? (long long)s_sq[0] : 0;
    stats[5] = 0; stats[6] = 0; stats[7] = 0;
    for (int j = 0; j < q.nq; ++j) {
      unsigned long long k = 0;
      unsigned r = 0;
      if (N) ih_rank(N, q.pn[j], q.pd[j], &k, &r);
      s_target[2 * j] = k;
      s_target[2 * j + 1] = N ? (k + 1 < N - 1 ? k + 1 : N - 1) : 0;
      stats[8 + 4 * j] = (long long)k; stats[9 + 4 * j] = (long long)r;
      if (!N) { stats[10 + 4 * j] = 0; stats[11 + 4 * j] = 0; }
    }
  }
  __syncthreads();
  if (N == 0 || cnt == 0) return;
  for (int e = 0; e < 2 * q.nq; ++e) {
    const unsigned long long tg = s_target[e];
    if (tg < excl || tg >= incl) continue;   // exactly one thread holds a rank < N
    unsigned long long acc = excl;
    for (int i = 0; i < PER; ++i) {
      acc += hist[base + i];
      if (tg < acc) { stats[8 + 4 * (e >> 1) + 2 + (e & 1)] = (long long)(base + i - IH_OFFSET); break; }
    }
  }
}

inline bool aligned_to(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

// persistent workgroups: one per CU (the LDS sub-histogram leaves room for no second one)
int hist_blocks(uint32_t nchunks, int* blocks) {
  static int cus = 0;
  if (cus <= 0) {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) {
      vu_set_error("intensity_hist: cannot read the number of compute units");
      return VU_ELAUNCH;
    }
    cus = n;
  }
  *blocks = (int)(nchunks < (uint32_t)cus ? nchunks : (uint32_t)cus);
  return VU_OK;
}

}  // namespace

extern "C" {

int vu_intensity_geometry(int* lds_base, int* lds_bins, int* voxels_per_block) {
  VU_REQUIRE(lds_base && lds_bins && voxels_per_block, "intensity_geometry: null argument");
  *lds_base = IH_LDS_BASE; *lds_bins = IH_LDS_BINS; *voxels_per_block = IH_V;
  return VU_OK;
}

int vu_intensity_hist(const int16_t* vol, const uint8_t* mask, uint32_t* hist, int32_t* bbox, int D, int H, int W, int select, int floor,
                      int label, void* stream) {
  VU_REQUIRE(vol && hist, "intensity_hist: null argument");
  VU_REQUIRE(select >= 0 && select <= 2, "intensity_hist: select must be 0 (all), 1 (above floor) or 2 (mask) (got %d)", select);
  VU_REQUIRE(select != 2 || mask, "intensity_hist: select 2 needs a mask");
  VU_REQUIRE(label <= 255, "intensity_hist: label must be negative (any non-zero mask value) or 0 .. 255 (got %d)", label);
  VU_REQUIRE(D >= 1 && H >= 1 && W >= 1, "intensity_hist: every dimension must be at least 1 (got %d x %d x %d)", D, H, W);
  const unsigned long long dh = (unsigned long long)D * (unsigned long long)H;   // < 2^62
  VU_REQUIRE(dh < (1ull << 32) && dh * (unsigned long long)W < (1ull << 32), "intensity_hist: 2^32 voxels or more (%d x %d x %d)", D, H, W);
  VU_REQUIRE(aligned_to(hist, 4) && (!bbox || aligned_to(bbox, 4)), "intensity_hist: hist and bbox must be 4-byte aligned");
  ih_args a;
  a.vol = vol; a.mask = select == 2 ? mask : nullptr; a.hist = hist; a.bbox = bbox;
  a.n = (uint32_t)(dh * (unsigned long long)W);
  a.nchunks = (uint32_t)(((unsigned long long)a.n + IH_V - 1) / IH_V);
  a.H = H; a.W = W; a.select = select; a.floor = floor; a.label = label;
  a.vec = (aligned_to(vol, 16) && (select != 2 || aligned_to(mask, 8))) ? 1 : 0;
  int blocks = 0;
  int rc = hist_blocks(a.nchunks, &blocks);
  if (rc) return rc;
  static bool reserved = false;
  if (!reserved) {
    if (IH_LDS_BYTES > 48 * 1024 &&
        hipFuncSetAttribute((const void*)intensity_hist_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)IH_LDS_BYTES) != hipSuccess) {
      vu_set_error("intensity_hist: cannot reserve %zu bytes of LDS", IH_LDS_BYTES);
      return VU_ELAUNCH;
    }
    reserved = true;
  }
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(intensity_clear_kernel, dim3(IH_BINS / IH_THREADS), dim3(IH_THREADS), 0, st, hist, bbox, D, H, W);
  rc = vu_check_launch("vu_intensity_hist/clear");
  if (rc) return rc;
  hipLaunchKernelGGL(intensity_hist_kernel, dim3(blocks), dim3(IH_THREADS), IH_LDS_BYTES, st, a);
  if (vu_prof_on()) vu_prof_note("intensity_hist_kernel", 0.0, (select == 2 ? 3.0 : 2.0) * a.n + 4.0 * IH_BINS);
  return vu_check_launch("vu_intensity_hist");
}

int vu_intensity_rank(unsigned long long N, unsigned pn, unsigned pd, unsigned long long* k, unsigned* r) {
  VU_REQUIRE(k && r, "intensity_rank: null argument");
  VU_REQUIRE(N >= 1 && N < (1ull << 32), "intensity_rank: N must be in 1 .. 2^32 - 1 (got %llu)", N);
  VU_REQUIRE(pd >= 1 && pd <= 1000000u && pn <= pd, "intensity_rank: the quantile needs 0 <= pn <= pd, 1 <= pd <= 10^6 (got %u / %u)", pn, pd);
  ih_rank(N, pn, pd, k, r);
  return VU_OK;
}

int vu_intensity_stats(const uint32_t* hist, const unsigned* pn, const unsigned* pd, int nq, long long* stats, void* stream) {
  VU_REQUIRE(hist && stats, "intensity_stats: null argument");
  VU_REQUIRE(nq >= 0 && nq <= 4, "intensity_stats: nq must be in 0 .. 4 (got %d)", nq);
  VU_REQUIRE(nq == 0 || (pn && pd), "intensity_stats: quantiles need pn and pd");
  ih_quantiles q = {{0u, 0u, 0u, 0u}, {1u, 1u, 1u, 1u}, nq};
  for (int j = 0; j < nq; ++j) {
    VU_REQUIRE(pd[j] >= 1 && pd[j] <= 1000000u && pn[j] <= pd[j],
               "intensity_stats: quantile %d needs 0 <= pn <= pd, 1 <= pd <= 10^6 (got %u / %u)", j, pn[j], pd[j]);
    q.pn[j] = pn[j]; q.pd[j] = pd[j];
  }
  VU_REQUIRE(aligned_to(hist, 4) && aligned_to(stats, 8), "intensity_stats: hist must be 4-byte, stats 8-byte aligned");
  hipLaunchKernelGGL(intensity_stats_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, hist, stats, q, aligned_to(hist, 16) ? 1 : 0);
  if (vu_prof_on()) vu_prof_note("intensity_stats_kernel", 0.0, 4.0 * IH_BINS + 8.0 * (8 + 4 * nq));
  return vu_check_launch("vu_intensity_stats");
}

}  // extern "C"
