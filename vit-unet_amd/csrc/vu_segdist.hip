// Surface-distance metrics for segmentation on the device: an exact Euclidean distance transform of a (D,H,W) uint8 mask, the
// MedPy / SciPy surface rule, and on top of both the per-unit numbers that the Hausdorff distance, its percentiles, the average
// symmetric surface distance and the surface Dice are made of.  Every device result except one float64 sum is an
// exact integer: spacings are integers, so the squared distance (sz dz)^2 + (sy dy)^2 + (sx dx)^2 is, and the entries refuse any
// volume whose largest possible value exceeds 2^31 - 1; 0xffffffff then means "no site in this unit".
//
// The transform is separable; the phases are separate launches (nothing waits on another workgroup):
//   (x) edt_x_kernel     one wave per row, 256 pixels (4 per lane) at a time: a forward scan leaves the index distance to the nearest
//                        site on the left, a backward scan takes the minimum with the one on the right and writes (sx dx)^2.  The
//                        nearest site inside the 256 pixels comes from one ballot and one lane read, the carry between them is a
//                        wave-uniform index.  Both scans have cdiv(W, 256) trips.
//   (y) edt_env_kernel   the lower envelope out[i] = min_j g[j] + (s (i - j))^2 along y: one workgroup owns EC = 64 neighbouring
//                        columns and EL = 128 consecutive outputs of each; a piece of EL inputs of those columns is staged in LDS
//                        (global accesses stay coalesced along x), lane = column, and every output walks outward from itself while
//                        (s d)^2 < best so far.  A line longer than EL is covered piece by piece, the workgroup's own piece first and
//                        then outward; a piece that cannot improve any output of the workgroup (a workgroup-wide vote) is not loaded.
//                        Between pieces an output lives in the destination buffer, read and written by the one thread that owns it.
//   (z) the same kernel along z (dims 3), its "columns" being the H W pixels of a slice.
// The passes alternate between the destination and one scratch buffer of the same size, so no pass works in place.
//
// vu_surface_dist: two surfaces, two transforms, then
//   sd_stats_kernel   per block of 1024 pixels of a unit: counts, maxima, counts within the tolerance, float64 sums of sqrt(d2),
//   sd_reduce_kernel  one block per unit sums the partials in a fixed order (the two-stage sum of vu_segtile.hip), writes stats and
//                     sums and the ranks of the six order statistics of the unit,
//   sd_hist_kernel /  radix select, 8 bits a pass from the top: a histogram of the next byte over the elements that still match
//   sd_scan_kernel    each statistic's prefix (LDS atomicAdd, then one global atomicAdd per non-empty bin), and a 256-bin walk
//                     that picks the bin holding the rank.  Four passes; integer sums do not depend on the order of arrival.
// No floating-point atomics anywhere: every output is the same bits on every run.
#include <stdio.h>
#include "vu_common.h"
#include "../../include/vit_unet_amd.h"

namespace {

constexpr uint32_t NOSITE = 0xffffffffu;
constexpr uint32_t FAR = 0x80000000u;   // "no site" inside the envelope pass: FAR + (s d)^2 <= 0xffffffff never wraps
constexpr int EL = 128, EC = 64;        // envelope pass: piece of a line in LDS, columns (lines) per workgroup
constexpr int XC = 256;                 // x pass: pixels a wave handles per trip
constexpr int SB = 1024;                // stats / histogram passes: pixels per block
constexpr int NSEL = 6;                 // order statistics per unit: (set 0, 1, 2) x (lo, hi)

__device__ __forceinline__ bool is_fg(unsigned v, int label) { return label < 0 ? v != 0u : v == (unsigned)label; }

// (x) row = blockIdx.x * 4 + wave.  out: uint32 (rows, W).  A wave never leaves before its last trip: every lane takes part in
// every ballot and lane read.
__global__ __launch_bounds__(256) void edt_x_kernel(const uint8_t* __restrict__ mask, uint32_t* out, long long rows, int W, int fg,
                                                    int sx, int vec_mask, int vec_out) {
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;   // the whole wave
  const int lane = threadIdx.x & 63;
  const uint8_t* m = mask + row * W;
  uint32_t* o = out + row * W;
  const int trips = (W + XC - 1) / XC;
  const unsigned long long below = (1ull << lane) - 1ull, above = ~((2ull << lane) - 1ull);

  auto sites = [&](int x0) -> unsigned {   // bit j: pixel x0 + j exists and is a site
    unsigned s = 0u;
    if (x0 + 3 < W && vec_mask) {
      const uint32_t u = *reinterpret_cast<const uint32_t*>(m + x0);
#pragma unroll
      for (int j = 0; j < 4; ++j) s |= ((((u >> (8 * j)) & 255u) != 0u) == (fg != 0)) ? (1u << j) : 0u;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (x0 + j < W) s |= ((m[x0 + j] != 0) == (fg != 0)) ? (1u << j) : 0u;
    }
    return s;
  };

  // forward: index distance to the nearest site at or left of the pixel
  int carry = -1;   // x of the last site of the trips before, wave-uniform
  for (int c = 0; c < trips; ++c) {
    const int x0 = c * XC + lane * 4;
    const unsigned s = sites(x0);
    const unsigned long long any = __ballot(s != 0u);
    const unsigned long long lo = any & below;
    const int pl = lo ? 63 - __builtin_clzll(lo) : 0;
    const unsigned sp = (unsigned)__shfl((int)s, pl, 64);
    const int left = lo ? c * XC + pl * 4 + (31 - __builtin_clz(sp)) : carry;
    uint32_t d[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned mj = s & ((2u << j) - 1u);
      const int pos = mj ? x0 + (31 - __builtin_clz(mj)) : left;
      d[j] = pos < 0 ? NOSITE : (uint32_t)(x0 + j - pos);
    }
    if (x0 + 3 < W && vec_out) {
      *reinterpret_cast<uint4*>(o + x0) = make_uint4(d[0], d[1], d[2], d[3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (x0 + j < W) o[x0 + j] = d[j];
    }
    const int ph = any ? 63 - __builtin_clzll(any) : 0;
    const unsigned sh = (unsigned)__shfl((int)s, ph, 64);
    if (any) carry = c * XC + ph * 4 + (31 - __builtin_clz(sh));
  }
  // backward: the minimum with the site at or right of the pixel; a lane reads back what it wrote itself
  carry = -1;
  for (int c = trips - 1; c >= 0; --c) {
    const int x0 = c * XC + lane * 4;
    const unsigned s = sites(x0);
    const unsigned long long any = __ballot(s != 0u);
    const unsigned long long hi = any & above;
    const int pr = hi ? __builtin_ctzll(hi) : 0;
    const unsigned sp = (unsigned)__shfl((int)s, pr, 64);
    const int right = hi ? c * XC + pr * 4 + __builtin_ctz(sp) : carry;
    uint32_t d[4] = {NOSITE, NOSITE, NOSITE, NOSITE};
    const bool full = x0 + 3 < W && vec_out;
    if (full) {
      const uint4 q = *reinterpret_cast<const uint4*>(o + x0);
      d[0] = q.x; d[1] = q.y; d[2] = q.z; d[3] = q.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (x0 + j < W) d[j] = o[x0 + j];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned mj = s >> j;
      const int pos = mj ? x0 + j + __builtin_ctz(mj) : right;
      const uint32_t dr = pos < 0 ? NOSITE : (uint32_t)(pos - (x0 + j));
      const uint32_t dm = dr < d[j] ? dr : d[j];
      const uint32_t sd = (uint32_t)sx * dm;   // <= sx (W - 1) <= 46340 where dm is a distance
      d[j] = dm == NOSITE ? NOSITE : sd * sd;
    }
    if (full) {
      *reinterpret_cast<uint4*>(o + x0) = make_uint4(d[0], d[1], d[2], d[3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (x0 + j < W) o[x0 + j] = d[j];
    }
    const int pf = any ? __builtin_ctzll(any) : 0;
    const unsigned sf = (unsigned)__shfl((int)s, pf, 64);
    if (any) carry = c * XC + pf * 4 + __builtin_ctz(sf);
  }
}

// (y), (z) blockIdx.x = (outer * nchunk + chunk) * ntx + tx.  Element j of column `col` of group `outer` is
// in[outer * outer_stride + j * line_stride + col]; L elements a line, ncol columns a group.  lane = column, wave w owns the
// outputs chunk * EL + w, + 4, ...  Trip counts: the piece loop 2 nchunk - 1, every walk at most EL.
__global__ __launch_bounds__(256) void edt_env_kernel(const uint32_t* __restrict__ in, uint32_t* out, long long outer_stride,
                                                      long long line_stride, int ncol, int L, int s, int ntx, int nchunk) {
  __shared__ uint32_t tile[EL * EC];
  const int tx = blockIdx.x % ntx;
  const int r = blockIdx.x / ntx;
  const int chunk = r % nchunk;
  const long long outer = r / nchunk;
  const int lx = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int col = tx * EC + lx;
  const bool col_in = col < ncol;
  const long long base = outer * outer_stride + col;
  const int i0 = chunk * EL, i1 = min(i0 + EL, L);   // the outputs of this workgroup
  uint32_t worst = 0u;   // the largest value among this thread's outputs so far
  for (int k = 0; k < 2 * nchunk - 1; ++k) {
    // own piece, then chunk - 1, chunk + 1, chunk - 2, ...
    const int dist = (k + 1) >> 1;
    const int p = (k & 1) ? chunk - dist : chunk + dist;
    if (p < 0 || p >= nchunk) continue;   // the same in every thread
    const int a = p * EL, b = min(a + EL, L);
    if (k > 0) {
      // every input of the piece is at least `gap` away from every output of the workgroup
      const uint32_t gap = (uint32_t)s * (uint32_t)(p > chunk ? a - (i1 - 1) : i0 - (b - 1));
      if (!__syncthreads_or(gap * gap < worst ? 1 : 0)) continue;   // the barrier also ends the reads of the piece before
    }
    for (int q = w; q < EL; q += 4) {
      uint32_t v = FAR;
      if (col_in && a + q < b) {
        v = in[base + (long long)(a + q) * line_stride];
        v = v > FAR ? FAR : v;
      }
      tile[q * EC + lx] = v;
    }
    __syncthreads();
    if (col_in) {
      for (int i = i0 + w; i < i1; i += 4) {
        uint32_t* dst = out + base + (long long)i * line_stride;
        uint32_t best = k == 0 ? NOSITE : *dst;
        if (i >= a && i < b) {
          const uint32_t c0 = tile[(i - a) * EC + lx];
          best = c0 < best ? c0 : best;
          const int dmax = max(i - a, b - 1 - i);
          for (int d = 1; d <= dmax; ++d) {
            const uint32_t sd = (uint32_t)s * (uint32_t)d, q2 = sd * sd;
            if (q2 >= best) break;
            if (i - d >= a) { const uint32_t c = tile[(i - d - a) * EC + lx] + q2; best = c < best ? c : best; }
            if (i + d < b) { const uint32_t c = tile[(i + d - a) * EC + lx] + q2; best = c < best ? c : best; }
          }
        } else if (i < a) {
          for (int j = a; j < b; ++j) {
            const uint32_t sd = (uint32_t)s * (uint32_t)(j - i), q2 = sd * sd;
            if (q2 >= best) break;
            const uint32_t c = tile[(j - a) * EC + lx] + q2;
            best = c < best ? c : best;
          }
        } else {
          for (int j = b - 1; j >= a; --j) {
            const uint32_t sd = (uint32_t)s * (uint32_t)(i - j), q2 = sd * sd;
            if (q2 >= best) break;
            const uint32_t c = tile[(j - a) * EC + lx] + q2;
            best = c < best ? c : best;
          }
        }
        best = best >= FAR ? NOSITE : best;
        *dst = best;
        if (k == 0) worst = best > worst ? best : worst;   // later pieces only lower an output
      }
    }
  }
}

// one thread per pixel: surf = foreground with an axis neighbour in the background or outside the unit
__global__ __launch_bounds__(256) void surface_kernel(const uint8_t* __restrict__ mask, uint8_t* __restrict__ surf, int D, int H, int W,
                                                      long long N, int dims3, int label) {
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  if (g >= N) return;
  const int x = (int)(g % W);
  const long long row = g / W;
  const int y = (int)(row % H), z = (int)(row / H);
  const long long hw = (long long)H * W;
  unsigned sv = 0u;
  if (is_fg(mask[g], label)) {
    bool inner = x > 0 && x < W - 1 && y > 0 && y < H - 1 && (!dims3 || (z > 0 && z < D - 1));
    if (inner) {
      inner = is_fg(mask[g - 1], label) && is_fg(mask[g + 1], label) && is_fg(mask[g - W], label) && is_fg(mask[g + W], label);
      if (inner && dims3) inner = is_fg(mask[g - hw], label) && is_fg(mask[g + hw], label);
    }
    sv = inner ? 0u : 1u;
  }
  surf[g] = (uint8_t)sv;
}

__device__ __forceinline__ unsigned wave_sum_u32(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}
__device__ __forceinline__ unsigned wave_max_u32(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned t = __shfl_down(v, o, 64);
    v = t > v ? t : v;
  }
  return v;
}
__device__ __forceinline__ double wave_sum_f64(double v) {   // a fixed tree
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// per-block partials, 8 x 8 bytes: |P|, |T|, max P->T, max T->P, within P->T, within T->P (uint64), sum P->T, sum T->P (double)
struct sd_partial { unsigned long long n[6]; double s[2]; };

// blockIdx.x = unit * bpu + block of the unit; thread t owns the pixels b SB + k 256 + t of its unit
__global__ __launch_bounds__(256) void sd_stats_kernel(const uint8_t* __restrict__ sp, const uint8_t* __restrict__ st,
                                                       const uint32_t* __restrict__ to_t, const uint32_t* __restrict__ to_p,
                                                       sd_partial* __restrict__ partials, long long unit_px, int bpu, uint32_t tol2) {
  __shared__ unsigned su[6][4];
  __shared__ double sf[2][4];
  const int u = blockIdx.x / bpu, b = blockIdx.x % bpu;
  const long long base = (long long)u * unit_px;
  unsigned c[6] = {0u, 0u, 0u, 0u, 0u, 0u};
  double f[2] = {0.0, 0.0};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const long long i = (long long)b * SB + k * 256 + threadIdx.x;
    if (i >= unit_px) continue;
    if (sp[base + i]) {
      const uint32_t v = to_t[base + i];
      ++c[0]; c[2] = v > c[2] ? v : c[2]; c[4] += v <= tol2 ? 1u : 0u; f[0] += sqrt((double)v);
    }
    if (st[base + i]) {
      const uint32_t v = to_p[base + i];
      ++c[1]; c[3] = v > c[3] ? v : c[3]; c[5] += v <= tol2 ? 1u : 0u; f[1] += sqrt((double)v);
    }
  }
  const int wv = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < 6; ++q) {
    const unsigned r = (q == 2 || q == 3) ? wave_max_u32(c[q]) : wave_sum_u32(c[q]);
    if ((threadIdx.x & 63) == 0) su[q][wv] = r;
  }
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const double r = wave_sum_f64(f[q]);
    if ((threadIdx.x & 63) == 0) sf[q][wv] = r;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    sd_partial p;
    for (int q = 0; q < 6; ++q) {
      unsigned r = su[q][0];
      for (int i = 1; i < 4; ++i) r = (q == 2 || q == 3) ? (su[q][i] > r ? su[q][i] : r) : r + su[q][i];
      p.n[q] = r;
    }
    for (int q = 0; q < 2; ++q) p.s[q] = ((sf[q][0] + sf[q][1]) + sf[q][2]) + sf[q][3];
    partials[blockIdx.x] = p;
  }
}

// selection state of one order statistic
struct sd_sel { uint32_t prefix, rank, live, pad; };

// one block per unit: thread i takes partials i, i + 256, ..., then a fixed tree over the 256 threads
__global__ __launch_bounds__(256) void sd_reduce_kernel(const sd_partial* __restrict__ partials, unsigned long long* __restrict__ stats,
                                                        double* __restrict__ sums, sd_sel* __restrict__ sel, int bpu, uint32_t qnum,
                                                        uint32_t qden) {
  __shared__ unsigned long long sn[6][256];
  __shared__ double sd[2][256];
  const sd_partial* p = partials + (size_t)blockIdx.x * bpu;
  unsigned long long n[6] = {0, 0, 0, 0, 0, 0};
  double f[2] = {0.0, 0.0};
  for (int i = threadIdx.x; i < bpu; i += 256) {
    for (int q = 0; q < 6; ++q) n[q] = (q == 2 || q == 3) ? (p[i].n[q] > n[q] ? p[i].n[q] : n[q]) : n[q] + p[i].n[q];
    f[0] += p[i].s[0]; f[1] += p[i].s[1];
  }
  for (int q = 0; q < 6; ++q) sn[q][threadIdx.x] = n[q];
  sd[0][threadIdx.x] = f[0]; sd[1][threadIdx.x] = f[1];
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      for (int q = 0; q < 6; ++q) {
        const unsigned long long a = sn[q][threadIdx.x], b = sn[q][threadIdx.x + o];
        sn[q][threadIdx.x] = (q == 2 || q == 3) ? (b > a ? b : a) : a + b;
      }
      sd[0][threadIdx.x] += sd[0][threadIdx.x + o];
      sd[1][threadIdx.x] += sd[1][threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const unsigned long long np = sn[0][0], nt = sn[1][0];
    const bool live = np > 0 && nt > 0;
    unsigned long long* s = stats + (size_t)blockIdx.x * 6;
    s[0] = np; s[1] = nt; s[2] = sn[2][0]; s[3] = sn[3][0];
    s[4] = live ? sn[4][0] : 0ull; s[5] = live ? sn[5][0] : 0ull;
    sums[(size_t)blockIdx.x * 2] = live ? sd[0][0] : 0.0;
    sums[(size_t)blockIdx.x * 2 + 1] = live ? sd[1][0] : 0.0;
    const unsigned long long cnt[3] = {np, nt, np + nt};
    for (int q = 0; q < 3; ++q) {
      sd_sel lo = {0u, 0u, live ? 1u : 0u, 0u}, hi = lo;
      if (live) {
        const unsigned long long l = ((unsigned long long)qnum * (cnt[q] - 1)) / qden;   // < 2^20 2^32
        lo.rank = (uint32_t)l;
        hi.rank = (uint32_t)(l + 1 < cnt[q] - 1 ? l + 1 : cnt[q] - 1);
      }
      sel[(size_t)blockIdx.x * NSEL + 2 * q] = lo;
      sel[(size_t)blockIdx.x * NSEL + 2 * q + 1] = hi;
    }
  }
}

// geometry of sd_stats_kernel.  hist (U, NSEL, 256) uint32, zero at entry.  An element counts for a statistic when its bits above
// `shift + 8` equal the statistic's prefix (keep = the mask of those bits, 0 in the first pass).
__global__ __launch_bounds__(256) void sd_hist_kernel(const uint8_t* __restrict__ sp, const uint8_t* __restrict__ st,
                                                      const uint32_t* __restrict__ to_t, const uint32_t* __restrict__ to_p,
                                                      const sd_sel* __restrict__ sel, uint32_t* hist, long long unit_px, int bpu,
                                                      int shift, uint32_t keep) {
  __shared__ unsigned h[NSEL][256];
  const int u = blockIdx.x / bpu, b = blockIdx.x % bpu;
  const sd_sel* se = sel + (size_t)u * NSEL;
  if (!se[0].live) return;   // the same in every thread: a unit is live or not as a whole
  uint32_t pre[NSEL];
#pragma unroll
  for (int q = 0; q < NSEL; ++q) { pre[q] = se[q].prefix; h[q][threadIdx.x] = 0u; }
  __syncthreads();
  const long long base = (long long)u * unit_px;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const long long i = (long long)b * SB + k * 256 + threadIdx.x;
    if (i >= unit_px) continue;
    if (sp[base + i]) {
      const uint32_t v = to_t[base + i], bin = (v >> shift) & 255u;
      if (((v ^ pre[0]) & keep) == 0u) atomicAdd(&h[0][bin], 1u);
      if (((v ^ pre[1]) & keep) == 0u) atomicAdd(&h[1][bin], 1u);
      if (((v ^ pre[4]) & keep) == 0u) atomicAdd(&h[4][bin], 1u);
      if (((v ^ pre[5]) & keep) == 0u) atomicAdd(&h[5][bin], 1u);
    }
    if (st[base + i]) {
      const uint32_t v = to_p[base + i], bin = (v >> shift) & 255u;
      if (((v ^ pre[2]) & keep) == 0u) atomicAdd(&h[2][bin], 1u);
      if (((v ^ pre[3]) & keep) == 0u) atomicAdd(&h[3][bin], 1u);
      if (((v ^ pre[4]) & keep) == 0u) atomicAdd(&h[4][bin], 1u);
      if (((v ^ pre[5]) & keep) == 0u) atomicAdd(&h[5][bin], 1u);
    }
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < NSEL; ++q) {
    const unsigned c = h[q][threadIdx.x];
    if (c) atomicAdd(&hist[((size_t)u * NSEL + q) * 256 + threadIdx.x], c);
  }
}

// one thread per statistic: the bin that holds the rank (256 trips), the bins zeroed for the next pass (256 trips); the last pass
// (shift 0) writes `order`
__global__ __launch_bounds__(256) void sd_scan_kernel(sd_sel* sel, uint32_t* hist, uint32_t* __restrict__ order, long long nsel, int shift) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= nsel) return;
  sd_sel s = sel[t];
  if (!s.live) {
    if (shift == 0) order[t] = NOSITE;
    return;
  }
  uint32_t* h = hist + (size_t)t * 256;
  uint32_t r = s.rank;
  int bin = 255;
  for (int q = 0; q < 256; ++q) {
    const uint32_t c = h[q];
    if (r < c) { bin = q; break; }
    r -= c;
  }
  for (int q = 0; q < 256; ++q) h[q] = 0u;
  s.prefix |= (uint32_t)bin << shift;
  s.rank = r;
  sel[t] = s;
  if (shift == 0) order[t] = s.prefix;
}

inline bool aligned_to(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

struct range { const void* p; size_t n; };
// true when two of the non-null ranges share a byte
bool any_overlap(const range* r, int n) {
  for (int i = 0; i < n; ++i)
    for (int j = i + 1; j < n; ++j) {
      if (!r[i].p || !r[j].p) continue;
      const uintptr_t a = (uintptr_t)r[i].p, b = (uintptr_t)r[j].p;
      if (a < b + r[j].n && b < a + r[i].n) return true;
    }
  return false;
}

// shape and unit checks shared by the entries; the messages carry the entry's name
int check_shape(const char* who, int D, int H, int W, int dims) {
  VU_REQUIRE(D > 0 && H > 0 && W > 0, "%s: empty volume (%d x %d x %d)", who, D, H, W);
  VU_REQUIRE(dims == 2 || dims == 3, "%s: dims must be 2 (slice by slice) or 3 (the volume) (got %d)", who, dims);
  VU_REQUIRE(!(dims == 3 && D == 1), "%s: dims 3 needs a volume, a single slice takes dims 2", who);
  VU_REQUIRE((long long)D * H * W <= 0x7fffffffLL, "%s: %d x %d x %d pixels exceed 2^31 - 1", who, D, H, W);
  return VU_OK;
}

// positive integer spacing, and the largest squared distance of a unit fits in 31 bits (so that every s d <= 46340 as well)
int check_spacing(const char* who, int D, int H, int W, int dims, int sz, int sy, int sx) {
  VU_REQUIRE(sz >= 1 && sy >= 1 && sx >= 1, "%s: the spacing must be positive integers (got %d, %d, %d)", who, sz, sy, sx);
  const long long t[3] = {dims == 3 ? (long long)sz * (D - 1) : 0LL, (long long)sy * (H - 1), (long long)sx * (W - 1)};
  long long sum = 0;
  for (int i = 0; i < 3; ++i) {
    if (t[i] > 46340) { sum = 0x80000000LL; break; }
    sum += t[i] * t[i];
  }
  VU_REQUIRE(sum <= 0x7fffffffLL, "%s: the largest squared distance exceeds 2^31 - 1 (spacing %d, %d, %d on %d x %d x %d)", who, sz, sy,
             sx, D, H, W);
  return VU_OK;
}

int env_launch(const char* what, const uint32_t* in, uint32_t* out, long long outer, long long outer_stride, long long line_stride,
               long long ncol, int L, int s, hipStream_t st) {
  const long long ntx = vu_cdiv64(ncol, EC), nchunk = vu_cdiv64(L, EL), nblk = ntx * nchunk * outer;
  VU_REQUIRE(nblk <= 0x7fffffffLL, "%s: launch too large", what);
  hipLaunchKernelGGL(edt_env_kernel, dim3((unsigned)nblk), dim3(256), 0, st, in, out, outer_stride, line_stride, (int)ncol, L, s, (int)ntx,
                     (int)nchunk);
  return vu_check_launch(what);
}

// the transform of `mask` into dist2; tmp: N uint32.  Arguments are checked by the caller.
int edt_launch(const char* who, const uint8_t* mask, uint32_t* dist2, uint32_t* tmp, int D, int H, int W, int dims, int fg, int sz, int sy,
               int sx, hipStream_t st) {
  const long long rows = (long long)D * H, hw = (long long)H * W;
  uint32_t* xo = dims == 3 ? dist2 : tmp;   // x -> y (-> z) alternate so that the last pass writes dist2
  uint32_t* yo = dims == 3 ? tmp : dist2;
  const int vec = W % 4 == 0 ? 1 : 0;
  char what[64];
  hipLaunchKernelGGL(edt_x_kernel, dim3((unsigned)vu_cdiv64(rows, 4)), dim3(256), 0, st, mask, xo, rows, W, fg, sx,
                     (vec && aligned_to(mask, 4)) ? 1 : 0, (vec && aligned_to(xo, 16)) ? 1 : 0);
  snprintf(what, sizeof what, "%s/x", who);
  int rc = vu_check_launch(what);
  if (rc) return rc;
  snprintf(what, sizeof what, "%s/y", who);
  rc = env_launch(what, xo, yo, D, hw, W, W, H, sy, st);
  if (rc || dims == 2) return rc;
  snprintf(what, sizeof what, "%s/z", who);
  return env_launch(what, yo, dist2, 1, 0, hw, hw, D, sz, st);
}

int surface_launch(const char* what, const uint8_t* mask, uint8_t* surf, int D, int H, int W, int dims, int label, hipStream_t st) {
  const long long N = (long long)D * H * W;
  hipLaunchKernelGGL(surface_kernel, dim3((unsigned)vu_cdiv64(N, 256)), dim3(256), 0, st, mask, surf, D, H, W, N, dims == 3 ? 1 : 0,
                     label);
  return vu_check_launch(what);
}

// scratch of vu_surface_dist: surface P | surface T | map to T | map to P | transform scratch | partials | selection state | histograms
struct sd_layout { size_t sp, st, to_t, to_p, tmp, partials, sel, hist, total; int U, bpu; long long unit_px; };
sd_layout make_layout(int D, int H, int W, int dims) {
  const size_t N = (size_t)D * H * W;
  sd_layout l;
  l.U = dims == 3 ? 1 : D;
  l.unit_px = dims == 3 ? (long long)N : (long long)H * W;
  l.bpu = (int)vu_cdiv64(l.unit_px, SB);
  l.sp = 0;
  l.st = vu_align_up(l.sp + N, 16);
  l.to_t = vu_align_up(l.st + N, 16);
  l.to_p = vu_align_up(l.to_t + N * 4, 16);
  l.tmp = vu_align_up(l.to_p + N * 4, 16);
  l.partials = vu_align_up(l.tmp + N * 4, 16);
  l.sel = l.partials + (size_t)l.U * l.bpu * sizeof(sd_partial);
  l.hist = l.sel + (size_t)l.U * NSEL * sizeof(sd_sel);
  l.total = l.hist + (size_t)l.U * NSEL * 256 * sizeof(uint32_t);
  return l;
}

}  // namespace

extern "C" {

int vu_segdist_geometry(int* line_piece, int* lines_per_group, int* row_chunk) {
  VU_REQUIRE(line_piece && lines_per_group && row_chunk, "segdist_geometry: null argument");
  *line_piece = EL;
  *lines_per_group = EC;
  *row_chunk = XC;
  return VU_OK;
}

size_t vu_edt_scratch_bytes(int D, int H, int W, int dims) {
  if (D <= 0 || H <= 0 || W <= 0 || (long long)D * H * W > 0x7fffffffLL || (dims != 2 && dims != 3)) return 0;
  return vu_align_up((size_t)D * H * W * 4, 16);
}

int vu_edt_sq(const uint8_t* mask, uint32_t* dist2, void* scratch, size_t scratch_bytes, int D, int H, int W, int dims, int fg, int sz,
              int sy, int sx, void* stream) {
  int rc = check_shape("edt_sq", D, H, W, dims);
  if (rc) return rc;
  rc = check_spacing("edt_sq", D, H, W, dims, sz, sy, sx);
  if (rc) return rc;
  VU_REQUIRE(fg == 0 || fg == 1, "edt_sq: fg must be 1 (sites are mask != 0) or 0 (sites are mask == 0) (got %d)", fg);
  VU_REQUIRE(mask && dist2 && scratch, "edt_sq: null argument (mask, dist2 and scratch are required)");
  const size_t N = (size_t)D * H * W, need = vu_edt_scratch_bytes(D, H, W, dims);
  VU_REQUIRE(scratch_bytes >= need && aligned_to(scratch, 4), "edt_sq: scratch too small or misaligned (%zu bytes needed, 4-byte aligned)",
             need);
  VU_REQUIRE(aligned_to(dist2, 4), "edt_sq: dist2 must be 4-byte aligned");
  const range r[3] = {{mask, N}, {dist2, N * 4}, {scratch, need}};
  VU_REQUIRE(!any_overlap(r, 3), "edt_sq: mask, dist2 and scratch must not overlap");
  return edt_launch("vu_edt_sq", mask, dist2, (uint32_t*)scratch, D, H, W, dims, fg, sz, sy, sx, (hipStream_t)stream);
}

int vu_mask_surface(const uint8_t* mask, uint8_t* surf, int D, int H, int W, int dims, int label, void* stream) {
  int rc = check_shape("mask_surface", D, H, W, dims);
  if (rc) return rc;
  VU_REQUIRE(label <= 255, "mask_surface: label must be negative (any non-zero pixel) or 0 .. 255 (got %d)", label);
  VU_REQUIRE(mask && surf, "mask_surface: null argument (mask and surf are required)");
  const size_t N = (size_t)D * H * W;
  const range r[2] = {{mask, N}, {surf, N}};
  VU_REQUIRE(!any_overlap(r, 2), "mask_surface: mask and surf must not overlap");
  return surface_launch("vu_mask_surface", mask, surf, D, H, W, dims, label, (hipStream_t)stream);
}

size_t vu_surface_dist_scratch_bytes(int D, int H, int W, int dims) {
  if (D <= 0 || H <= 0 || W <= 0 || (long long)D * H * W > 0x7fffffffLL || (dims != 2 && dims != 3)) return 0;
  return make_layout(D, H, W, dims).total;
}

int vu_surface_dist(const uint8_t* pred, const uint8_t* truth, unsigned long long* stats, double* sums, uint32_t* order,
                    uint32_t* dist_pt, uint32_t* dist_tp, void* scratch, size_t scratch_bytes, int D, int H, int W, int dims, int sz,
                    int sy, int sx, int label, uint32_t tol2, uint32_t qnum, uint32_t qden, void* stream) {
  int rc = check_shape("surface_dist", D, H, W, dims);
  if (rc) return rc;
  rc = check_spacing("surface_dist", D, H, W, dims, sz, sy, sx);
  if (rc) return rc;
  VU_REQUIRE(label <= 255, "surface_dist: label must be negative (any non-zero truth) or 0 .. 255 (got %d)", label);
  VU_REQUIRE(qden >= 1 && qden <= 1000000u && qnum <= qden, "surface_dist: the quantile needs 0 <= qnum <= qden, 1 <= qden <= 1000000 (got %u / %u)",
             qnum, qden);
  VU_REQUIRE(pred && truth && stats && sums && order && scratch,
             "surface_dist: null argument (pred, truth, stats, sums, order and scratch are required)");
  const size_t N = (size_t)D * H * W;
  const sd_layout lay = make_layout(D, H, W, dims);
  VU_REQUIRE(scratch_bytes >= lay.total && aligned_to(scratch, 16),
             "surface_dist: scratch too small or misaligned (%zu bytes needed, 16-byte aligned)", lay.total);
  VU_REQUIRE(aligned_to(stats, 8) && aligned_to(sums, 8) && aligned_to(order, 4) && aligned_to(dist_pt, 4) && aligned_to(dist_tp, 4),
             "surface_dist: stats and sums must be 8-byte, order and the maps 4-byte aligned");
  const size_t U = (size_t)lay.U;
  const range r[8] = {{pred, N}, {truth, N}, {stats, U * 48}, {sums, U * 16}, {order, U * 24}, {dist_pt, N * 4}, {dist_tp, N * 4},
                      {scratch, lay.total}};
  // the two inputs may be one buffer (a mask scored against itself); nothing else may share a byte
  const range rin[7] = {{pred, N}, r[2], r[3], r[4], r[5], r[6], r[7]};
  VU_REQUIRE(!any_overlap(r + 1, 7) && !any_overlap(rin, 7) && (pred == truth || !any_overlap(r, 2)),
             "surface_dist: the outputs and the scratch must not overlap each other or the inputs (pred may be truth itself)");
  const long long nblk = (long long)lay.U * lay.bpu, nsel = (long long)lay.U * NSEL;
  VU_REQUIRE(nblk <= 0x7fffffffLL, "surface_dist: launch too large (%d slices of %d x %d)", D, H, W);

  hipStream_t st = (hipStream_t)stream;
  char* base = (char*)scratch;
  uint8_t* sp = (uint8_t*)(base + lay.sp);
  uint8_t* stt = (uint8_t*)(base + lay.st);
  uint32_t* to_t = dist_pt ? dist_pt : (uint32_t*)(base + lay.to_t);
  uint32_t* to_p = dist_tp ? dist_tp : (uint32_t*)(base + lay.to_p);
  uint32_t* tmp = (uint32_t*)(base + lay.tmp);
  sd_partial* partials = (sd_partial*)(base + lay.partials);
  sd_sel* sel = (sd_sel*)(base + lay.sel);
  uint32_t* hist = (uint32_t*)(base + lay.hist);
  if (hipMemsetAsync(hist, 0, lay.total - lay.hist, st) != hipSuccess) {
    vu_set_error("surface_dist: clearing the scratch failed: %s", hipGetErrorString(hipGetLastError()));
    return VU_ELAUNCH;
  }
  rc = surface_launch("vu_surface_dist/surface_p", pred, sp, D, H, W, dims, -1, st);
  if (rc) return rc;
  rc = surface_launch("vu_surface_dist/surface_t", truth, stt, D, H, W, dims, label, st);
  if (rc) return rc;
  rc = edt_launch("vu_surface_dist/edt_t", stt, to_t, tmp, D, H, W, dims, 1, sz, sy, sx, st);
  if (rc) return rc;
  rc = edt_launch("vu_surface_dist/edt_p", sp, to_p, tmp, D, H, W, dims, 1, sz, sy, sx, st);
  if (rc) return rc;
  hipLaunchKernelGGL(sd_stats_kernel, dim3((unsigned)nblk), dim3(256), 0, st, (const uint8_t*)sp, (const uint8_t*)stt,
                     (const uint32_t*)to_t, (const uint32_t*)to_p, partials, lay.unit_px, lay.bpu, tol2);
  rc = vu_check_launch("vu_surface_dist/stats");
  if (rc) return rc;
  hipLaunchKernelGGL(sd_reduce_kernel, dim3((unsigned)lay.U), dim3(256), 0, st, (const sd_partial*)partials, stats, sums, sel, lay.bpu,
                     qnum, qden);
  rc = vu_check_launch("vu_surface_dist/reduce");
  if (rc) return rc;
  for (int shift = 24; shift >= 0; shift -= 8) {
    const uint32_t keep = shift == 24 ? 0u : 0xffffffffu << (shift + 8);
    hipLaunchKernelGGL(sd_hist_kernel, dim3((unsigned)nblk), dim3(256), 0, st, (const uint8_t*)sp, (const uint8_t*)stt,
                       (const uint32_t*)to_t, (const uint32_t*)to_p, (const sd_sel*)sel, hist, lay.unit_px, lay.bpu, shift, keep);
    rc = vu_check_launch("vu_surface_dist/hist");
    if (rc) return rc;
    hipLaunchKernelGGL(sd_scan_kernel, dim3((unsigned)vu_cdiv64(nsel, 256)), dim3(256), 0, st, sel, hist, order, nsel, shift);
    rc = vu_check_launch("vu_surface_dist/scan");
    if (rc) return rc;
  }
  return VU_OK;
}

}  // extern "C"
