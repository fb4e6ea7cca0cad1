// Segmentation mask clean-up on the device: connected-component labelling of a (D,H,W) uint8 mask and, on top of it, the three
// steps every organ-segmentation pipeline applies between the threshold and the reported score - drop small components, keep the
// largest one, fill enclosed holes - ending in the per-slice integer counts of csrc/vu_segtile.hip.
//
// Labelling is a union-find over the linear pixel index i = (z H + y) W + x; a parent is never larger than its child, so the root
// of a component is its smallest index.  The label array itself is the parent array; the phases are separate launches (kernel
// boundaries are the only ordering between workgroups, nothing waits on anything):
//   (a) cc_tile_kernel     one workgroup per TH x TW tile: union-find in LDS over the in-slice connectivity (LDS atomicMin).  A
//                          local root writes its own index, every other pixel -(index of its local root) - 2, background -1; the
//                          tile's part of `sizes` is zeroed.  So "value >= 0" means "root node" from here on, and only root
//                          entries are ever read or changed by another workgroup.
//   (b) cc_merge_kernel    pixels on tile edges unite with their neighbours across the edge, for conn 6 / 26 every pixel also with
//                          its 1 / 9 neighbours in the slice below: lock-free union, atomicMin on the larger root.  Every access to
//                          the label array in this launch is an agent-scope relaxed atomic (a plain load of another workgroup's
//                          write is not seen across XCDs); parents only decrease, so a stale read costs a retry, never the result.
//   (c)  cc_compress_kernel  every former local root takes its final root (halving find, atomics only), so that no path is longer
//                          than two entries afterwards.
//   (c,d) cc_flatten_kernel  one workgroup per tile again: every pixel takes the root of its local root; pixel counts and the
//                          touches-the-unit-border flag are summed per LOCAL root in LDS, then one global atomicAdd (and at most
//                          one atomicOr) per tile and local component - a large organ does not add pixel by pixel to one address.
//   (e) clean_select_kernel  per unit: components found, components of at least min_size, and a 64-bit atomicMax of
//                          (size << 32) | ~root - the largest component, ties to the smallest root - after a block reduction.
//   (f) clean_write_kernel   the cleaned mask (4 bytes per thread where aligned) and per-block partial counts; clean_counts_kernel
//                          sums them per slice in a fixed order (the two-stage sum of vu_segtile.hip).
// Integer atomic sums, minima, maxima and ors do not depend on the order of arrival: every output is the same bits on every run.
//
// Every data-dependent loop has an iteration cap derived from a bound (below, at each loop); a loop that reaches its cap sets the
// overflow word and leaves.  Independently of the caps every step of a find moves to a strictly smaller, non-negative index, so no
// loop can cycle or read outside the array whatever the array holds.
#include <stdio.h>
#include "vu_common.h"
#include "../../include/vit_unet_amd.h"

namespace {

constexpr int TH = 16, TW = 64, TPIX = TH * TW;   // 256 threads, one thread = 4 consecutive pixels of a tile row
constexpr unsigned BORDER = 0x80000000u;          // bit 31 of a size word: the component touches a border of its unit (sizes < 2^31)

__device__ __forceinline__ int lds_ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ int g_ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void set_overflow(unsigned* ovf) { __hip_atomic_fetch_or(ovf, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// LDS find.  Bound: a path visits strictly decreasing local indices, all below TPIX, so at most TPIX reads.
__device__ __forceinline__ int lds_find(const int* lab, int x, unsigned* ovf) {
  for (int i = 0; i < TPIX; ++i) {
    const int p = lds_ld(lab + x);
    if (p == x) return x;
    if (p < 0 || p > x) break;
    x = p;
  }
  set_overflow(ovf);
  return x;
}

// LDS union.  Bound: a failed atomicMin returns a parent smaller than the larger root, which replaces it: the larger of the two
// nodes strictly decreases from below TPIX, so at most TPIX attempts.
__device__ __forceinline__ void lds_union(int* lab, int a, int b, unsigned* ovf) {
  for (int i = 0; i < TPIX; ++i) {
    a = lds_find(lab, a, ovf);
    b = lds_find(lab, b, ovf);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = __hip_atomic_fetch_min(lab + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (old == a) return;
    if (old < 0 || old > a) break;
    a = old;
  }
  set_overflow(ovf);
}

// Global find over root nodes.  Bound (`cap`, from the host): a path visits strictly decreasing root nodes, each the local root of
// one local component of one tile of the unit; a tile has at most TPIX / 2 local components (one pixel of each is an independent
// set of the grid graph), so at most 1 + tiles-of-the-unit * TPIX / 2 reads.
// HALVE (the merge launch only, where every access is atomic): a node whose parent is not a root is handed its grandparent with
// the same atomicMin - an ancestor and smaller, so every invariant holds; it shortens the chains the serpentine cases build and
// changes no result.  The flatten launch, whose owners write final roots with plain stores, only reads.
template <bool HALVE>
__device__ __forceinline__ int g_find(int* labels, int x, int cap, unsigned* ovf) {
  for (int i = 0; i < cap; ++i) {
    const int p = g_ld(labels + x);
    if (p == x) return x;
    if (p < 0 || p > x) break;
    const int gp = g_ld(labels + p);
    if (gp == p) return p;
    if (gp < 0 || gp > p) break;
    if (HALVE) __hip_atomic_fetch_min(labels + x, gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    x = gp;
  }
  set_overflow(ovf);
  return x;
}

// Global union, the same argument as lds_union with the bound of g_find.  Returns a node of the united tree (the smaller root).
__device__ __forceinline__ int g_union(int* labels, int a, int b, int cap, unsigned* ovf) {
  for (int i = 0; i < cap; ++i) {
    a = g_find<true>(labels, a, cap, ovf);
    b = g_find<true>(labels, b, cap, ovf);
    if (a == b) return a;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = __hip_atomic_fetch_min(labels + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old == a) return b;
    if (old < 0 || old > a) break;
    a = old;
  }
  set_overflow(ovf);
  return b;
}

// the node a pixel starts from: itself when its entry is a root entry, else the local root its entry names
__device__ __forceinline__ int node_of(int v, int g) { return v >= 0 ? g : -(v + 2); }

struct tile_pos { int z, ty, tx; };
__device__ __forceinline__ tile_pos tile_of_block(int tiles_y, int tiles_x) {
  tile_pos t;
  t.tx = blockIdx.x % tiles_x;
  const int r = blockIdx.x / tiles_x;
  t.ty = r % tiles_y;
  t.z = r / tiles_y;
  return t;
}

// (a) blockIdx.x = (z tiles_y + ty) tiles_x + tx
__global__ __launch_bounds__(256) void cc_tile_kernel(const uint8_t* __restrict__ mask, int* __restrict__ labels,
                                                      uint32_t* __restrict__ sizes, unsigned* ovf, int H, int W, int tiles_y,
                                                      int tiles_x, int fg, int conn8, int vec_mask, int vec_lab, int vec_sizes) {
  __shared__ int lab[TPIX];
  const tile_pos t = tile_of_block(tiles_y, tiles_x);
  const int ly = threadIdx.x >> 4, lx0 = (threadIdx.x & 15) << 2;
  const int y = t.ty * TH + ly, x0 = t.tx * TW + lx0;
  const bool row_in = y < H, full = row_in && x0 + 3 < W;
  const long long g0 = ((long long)t.z * H + y) * W + x0;   // < 2^31 wherever a pixel exists
  unsigned m[4] = {0u, 0u, 0u, 0u};
  if (full && vec_mask) {
    const uint32_t u = *reinterpret_cast<const uint32_t*>(mask + g0);
    m[0] = u & 255u; m[1] = (u >> 8) & 255u; m[2] = (u >> 16) & 255u; m[3] = u >> 24;
  } else if (row_in) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (x0 + j < W) m[j] = mask[g0 + j];
  }
  const int l0 = ly * TW + lx0;
  bool f[4];
  int li[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    f[j] = row_in && x0 + j < W && ((m[j] != 0u) == (fg != 0));
    // a pixel starts at the first pixel of its run inside the thread's quad
    li[j] = !f[j] ? -1 : (j > 0 && f[j - 1]) ? li[j - 1] : l0 + j;
    lab[l0 + j] = li[j];
  }
  __syncthreads();
  // unions with the neighbours before the pixel in raster order; an entry >= 0 is a labelled pixel at any time
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (!f[j]) continue;
    const int l = l0 + j, lx = lx0 + j;
    if (j == 0 && lx > 0 && lds_ld(lab + l - 1) >= 0) lds_union(lab, l, l - 1, ovf);
    if (ly > 0) {
      if (lds_ld(lab + l - TW) >= 0) {
        lds_union(lab, l, l - TW, ovf);   // the diagonal neighbours are row neighbours of this one
      } else if (conn8) {
        if (lx > 0 && lds_ld(lab + l - TW - 1) >= 0) lds_union(lab, l, l - TW - 1, ovf);
        if (lx < TW - 1 && lds_ld(lab + l - TW + 1) >= 0) lds_union(lab, l, l - TW + 1, ovf);
      }
    }
  }
  __syncthreads();
  int v[4];
  const long long tile0 = ((long long)t.z * H + t.ty * TH) * W + t.tx * TW;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    v[j] = -1;
    if (f[j]) {
      const int r = lds_find(lab, l0 + j, ovf);
      const long long gr = tile0 + (long long)(r / TW) * W + (r % TW);
      v[j] = r == l0 + j ? (int)(g0 + j) : (int)(-(gr + 2));
    }
  }
  if (full && vec_lab) {
    *reinterpret_cast<int4*>(labels + g0) = make_int4(v[0], v[1], v[2], v[3]);
  } else if (row_in) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (x0 + j < W) labels[g0 + j] = v[j];
  }
  if (sizes) {
    if (full && vec_sizes) {
      *reinterpret_cast<uint4*>(sizes + g0) = make_uint4(0u, 0u, 0u, 0u);
    } else if (row_in) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (x0 + j < W) sizes[g0 + j] = 0u;
    }
  }
}

// (b) one thread per pixel; all but the pixels on a tile edge (and, conn 6 / 26, all of slice 0) leave at once
__global__ __launch_bounds__(256) void cc_merge_kernel(int* labels, unsigned* ovf, int H, int W, long long N, int conn, int cap) {
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= N) return;
  const int x = (int)(gid % W);
  const long long row = gid / W;
  const int y = (int)(row % H), z = (int)(row / H);
  const bool conn3 = conn == 6 || conn == 26, c8 = conn == 8 || conn == 26;
  const int lx = x % TW, ly = y % TH;
  const bool edge = lx == 0 || ly == 0 || (c8 && lx == TW - 1), below = conn3 && z > 0;
  if (!edge && !below) return;
  const int g = (int)gid;
  const int v = g_ld(labels + g);
  if (v == -1) return;
  int a = node_of(v, g);
  auto unite = [&](int q) {
    const int vq = g_ld(labels + q);
    if (vq != -1) a = g_union(labels, a, node_of(vq, q), cap, ovf);
  };
  if (edge) {
    if (lx == 0 && x > 0) unite(g - 1);
    if (y > 0) {
      const bool up = g_ld(labels + g - W) != -1;
      if (up) {
        if (ly == 0) unite(g - W);   // its row neighbours are united with it by their own threads or in LDS
      } else if (c8) {
        if (x > 0 && (lx == 0 || ly == 0)) unite(g - W - 1);
        if (x < W - 1 && (ly == 0 || lx == TW - 1)) unite(g - W + 1);
      }
    }
  }
  if (below) {
    const int b = g - H * W;
    if (conn == 6 || g_ld(labels + b) != -1) {
      unite(b);   // conn 26: the other eight are in-slice neighbours of this one, united with it in their own slice
    } else {
      for (int dy = -1; dy <= 1; ++dy) {
        if (y + dy < 0 || y + dy >= H) continue;
        for (int dx = -1; dx <= 1; ++dx)
          if (x + dx >= 0 && x + dx < W) unite(b + dy * W + dx);
      }
    }
  }
}

// (c) first half: after (b) no root changes any more, so every former local root (entry >= 0, not its own) takes its final root
// by the same halving find and atomicMin - atomics only, as in (b).  The flatten launch then reads paths of at most two entries.
__global__ __launch_bounds__(256) void cc_compress_kernel(int* labels, unsigned* ovf, long long N, int cap) {
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= N) return;
  const int g = (int)gid;
  const int v = labels[g];   // own entry; "root entry or not" was settled by (a)
  if (v < 0 || v == g) return;
  const int r = g_find<true>(labels, g, cap, ovf);
  __hip_atomic_fetch_min(labels + g, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// (c,d) the geometry of (a).  Entries of other pixels are only read where they are root entries, and a root entry holds a node of
// its own tree before and after its owner has written the root into it.
__global__ __launch_bounds__(256) void cc_flatten_kernel(int* labels, uint32_t* sizes, unsigned* ovf, int D, int H, int W,
                                                         int tiles_y, int tiles_x, int conn3, int want_flags, int cap, int vec_lab) {
  __shared__ unsigned cnt[TPIX];
  const tile_pos t = tile_of_block(tiles_y, tiles_x);
  const int ly = threadIdx.x >> 4, lx0 = (threadIdx.x & 15) << 2;
  const int y = t.ty * TH + ly, x0 = t.tx * TW + lx0;
  const bool row_in = y < H, full = row_in && x0 + 3 < W;
  const long long g0 = ((long long)t.z * H + y) * W + x0;
  const long long tile0 = ((long long)t.z * H + t.ty * TH) * W + t.tx * TW;
  int v[4] = {-1, -1, -1, -1};
  if (full && vec_lab) {
    const int4 q = *reinterpret_cast<const int4*>(labels + g0);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else if (row_in) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (x0 + j < W) v[j] = labels[g0 + j];
  }
  if (sizes) {
#pragma unroll
    for (int j = 0; j < 4; ++j) cnt[ly * TW + lx0 + j] = 0u;
    __syncthreads();
  }
  int R[4] = {-1, -1, -1, -1};
  int prev_node = -1, prev_root = -1, prev_ll = 0;
  unsigned run = 0u;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (v[j] == -1) continue;
    const int g = (int)(g0 + j), nd = node_of(v[j], g);
    R[j] = prev_root = nd == prev_node ? prev_root : g_find<false>(labels, nd, cap, ovf);
    if (sizes) {
      if (nd != prev_node) {
        if (run) atomicAdd(&cnt[prev_ll], run);
        const long long rel = nd - tile0;          // the local root lies in this tile
        prev_ll = (int)(rel / W) * TW + (int)(rel % W);
        run = 0u;
      }
      ++run;
      const int x = x0 + j;
      if (want_flags && (x == 0 || x == W - 1 || y == 0 || y == H - 1 || (conn3 && (t.z == 0 || t.z == D - 1))))
        atomicOr(&cnt[prev_ll], BORDER);
    }
    prev_node = nd;
  }
  if (sizes) {
    if (run) atomicAdd(&cnt[prev_ll], run);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (v[j] < 0) continue;                       // local roots only: one global add per tile and local component
      const unsigned c = cnt[ly * TW + lx0 + j];
      atomicAdd(&sizes[R[j]], c & ~BORDER);
      if (c & BORDER) atomicOr(&sizes[R[j]], BORDER);
    }
  }
  if (full && vec_lab) {
    *reinterpret_cast<int4*>(labels + g0) = make_int4(R[0], R[1], R[2], R[3]);
  } else if (row_in) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (x0 + j < W) labels[g0 + j] = R[j];
  }
}

__device__ __forceinline__ unsigned wave_sum_u32(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long w = __shfl_down(v, o, 64);
    v = w > v ? w : v;
  }
  return v;
}

// (e) blockIdx.x = unit * bpu + block of the unit (1024 pixels a block).  acc (U,4) uint64, zeroed: found, of at least min_size,
// max of (size << 32) | ~root, unused.
__global__ __launch_bounds__(256) void clean_select_kernel(const uint32_t* __restrict__ sizes, unsigned long long* acc, long long unit_px,
                                                           int bpu, unsigned min_size) {
  __shared__ unsigned sf[4], sg[4];
  __shared__ unsigned long long sb[4];
  const int u = blockIdx.x / bpu, b = blockIdx.x % bpu;
  const long long base = (long long)u * unit_px;
  unsigned found = 0u, ge = 0u;
  unsigned long long best = 0ull;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const long long i = (long long)b * 1024 + k * 256 + threadIdx.x;
    if (i >= unit_px) continue;
    const unsigned s = sizes[base + i] & ~BORDER;
    if (!s) continue;
    ++found;
    ge += s >= min_size ? 1u : 0u;
    const unsigned long long key = ((unsigned long long)s << 32) | (unsigned)~(unsigned)(base + i);
    best = key > best ? key : best;
  }
  found = wave_sum_u32(found);
  ge = wave_sum_u32(ge);
  best = wave_max_u64(best);
  const int wv = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { sf[wv] = found; sg[wv] = ge; sb[wv] = best; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned F = sf[0] + sf[1] + sf[2] + sf[3], G = sg[0] + sg[1] + sg[2] + sg[3];
    unsigned long long B = sb[0];
    for (int i = 1; i < 4; ++i) B = sb[i] > B ? sb[i] : B;
    if (F) {
      atomicAdd(&acc[4 * u], (unsigned long long)F);
      if (G) atomicAdd(&acc[4 * u + 1], (unsigned long long)G);
      atomicMax(&acc[4 * u + 2], B);
    }
  }
}

// (f) the geometry of seg_blend_kernel: one thread = 4 consecutive pixels of one row of one slice, blockIdx.x = slice * nb + block.
// FILL 0: out = the pixel's component survives steps 2 and 3.  FILL 1: out = inter | the pixel's background component touches no
// border (labels / sizes are those of the background of `inter`, which may be `out`: a thread reads its own quad before it writes).
template <int FILL>
__global__ __launch_bounds__(256) void clean_write_kernel(const int* __restrict__ labels, const uint32_t* __restrict__ sizes,
                                                          const unsigned long long* __restrict__ acc, const uint8_t* inter,
                                                          const uint8_t* __restrict__ truth, uint8_t* out, uint32_t* __restrict__ partials,
                                                          int H, int W, int nb, int per_slice, int conn3, unsigned min_size,
                                                          int keep_largest, int label, int vec_lab, int vec_out, int vec_truth) {
  __shared__ unsigned sm[2][4];
  const int zs = blockIdx.x / nb, bs = blockIdx.x % nb;
  const int lid = bs * 256 + threadIdx.x;
  unsigned c_pred = 0, c_true = 0, c_both = 0;
  if (lid < per_slice) {
    const int nq = (W + 3) >> 2;
    const int y = lid / nq, x0 = (lid % nq) * 4;
    const bool full = x0 + 3 < W;
    const size_t o = ((size_t)zs * H + y) * W + x0;
    int l[4] = {-1, -1, -1, -1};
    if (vec_lab && full) {
      const int4 q = *reinterpret_cast<const int4*>(labels + o);
      l[0] = q.x; l[1] = q.y; l[2] = q.z; l[3] = q.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (x0 + j < W) l[j] = labels[o + j];
    }
    unsigned m[4] = {0u, 0u, 0u, 0u};
    if (FILL) {
      if (vec_out && full) {
        const uint32_t u = *reinterpret_cast<const uint32_t*>(inter + o);
        m[0] = u & 255u; m[1] = (u >> 8) & 255u; m[2] = (u >> 16) & 255u; m[3] = u >> 24;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (x0 + j < W) m[j] = inter[o + j];
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (x0 + j < W && !m[j] && l[j] >= 0) m[j] = (sizes[l[j]] & BORDER) ? 0u : 1u;
    } else {
      const unsigned long long w = acc[4 * (conn3 ? 0 : zs) + 2];
      const unsigned wsize = (unsigned)(w >> 32);
      const int wroot = (wsize > 0u && wsize >= min_size) ? (int)~(unsigned)w : -1;   // no component left: nothing is kept
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (l[j] >= 0) m[j] = (keep_largest ? l[j] == wroot : (sizes[l[j]] & ~BORDER) >= min_size) ? 1u : 0u;
    }
    if (vec_out && full) {
      *reinterpret_cast<uint32_t*>(out + o) = m[0] | (m[1] << 8) | (m[2] << 16) | (m[3] << 24);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (x0 + j < W) out[o + j] = (uint8_t)m[j];
    }
    if (partials) {
      unsigned tv[4] = {0u, 0u, 0u, 0u};
      if (vec_truth && full) {
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

// one block per slice: thread i sums partials i, i + 256, ..., then a fixed tree over the 256 threads (seg_counts_kernel)
__global__ __launch_bounds__(256) void clean_counts_kernel(const uint32_t* __restrict__ partials, unsigned long long* __restrict__ counts,
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

// stats (U,4) int64: found, kept after step 3, size of the largest component found, overflow
__global__ void clean_stats_kernel(const unsigned long long* __restrict__ acc, const unsigned* __restrict__ ovf, long long* stats, int U,
                                   unsigned min_size, int keep_largest) {
  const int u = blockIdx.x * 256 + threadIdx.x;
  if (u >= U) return;
  const unsigned long long ge = acc[4 * u + 1], largest = acc[4 * u + 2] >> 32;
  stats[4 * u] = (long long)acc[4 * u];
  stats[4 * u + 1] = (long long)(keep_largest ? (largest > 0 && largest >= min_size ? 1ull : 0ull) : ge);
  stats[4 * u + 2] = (long long)largest;
  stats[4 * u + 3] = (long long)*ovf;
}

inline bool aligned_to(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
inline bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + nb && b0 < a0 + na;
}
inline long long blocks_per_slice(int H, int W) { return vu_cdiv64((long long)H * ((W + 3) / 4), 256); }
inline bool conn_ok(int conn) { return conn == 4 || conn == 8 || conn == 6 || conn == 26; }
inline int dual_conn(int conn) { return conn == 4 ? 8 : conn == 8 ? 4 : conn == 6 ? 26 : 6; }

// shape checks shared by both entries; the messages carry the entry's name
int check_shape(const char* who, int D, int H, int W, int conn) {
  VU_REQUIRE(D > 0 && H > 0 && W > 0, "%s: empty volume (%d x %d x %d)", who, D, H, W);
  VU_REQUIRE(conn_ok(conn), "%s: connectivity must be 4 or 8 (slice by slice), 6 or 26 (the volume) (got %d)", who, conn);
  VU_REQUIRE(!((conn == 6 || conn == 26) && D == 1), "%s: connectivity %d needs a volume, a single slice takes 4 or 8", who, conn);
  VU_REQUIRE((long long)D * H * W <= 0x7fffffffLL, "%s: %d x %d x %d pixels exceed 2^31 - 1", who, D, H, W);
  return VU_OK;
}

// phases (a) - (c,d); `ovf` zeroed by the caller.  sizes may be null (then no flags either).
int label_launch(const char* who, const uint8_t* mask, int* labels, uint32_t* sizes, unsigned* ovf, int D, int H, int W, int conn,
                 int fg, int want_flags, hipStream_t st) {
  const int tiles_y = vu_cdiv(H, TH), tiles_x = vu_cdiv(W, TW);
  const long long tiles_unit = (long long)tiles_y * tiles_x * ((conn == 6 || conn == 26) ? D : 1);
  const long long N = (long long)D * H * W, nblk = (long long)tiles_y * tiles_x * D;
  const long long cap64 = 1 + tiles_unit * (TPIX / 2);
  const int cap = cap64 > 0x7fffffffLL ? 0x7fffffff : (int)cap64;
  const int conn8 = (conn == 8 || conn == 26) ? 1 : 0, conn3 = (conn == 6 || conn == 26) ? 1 : 0;
  const int vec = W % 4 == 0 ? 1 : 0;
  const int vec_mask = (vec && aligned_to(mask, 4)) ? 1 : 0, vec_lab = (vec && aligned_to(labels, 16)) ? 1 : 0;
  const int vec_sizes = (vec && sizes && aligned_to(sizes, 16)) ? 1 : 0;
  char what[64];
  hipLaunchKernelGGL(cc_tile_kernel, dim3((unsigned)nblk), dim3(256), 0, st, mask, labels, sizes, ovf, H, W, tiles_y, tiles_x, fg,
                     conn8, vec_mask, vec_lab, vec_sizes);
  snprintf(what, sizeof what, "%s/tile", who);
  int rc = vu_check_launch(what);
  if (rc) return rc;
  if (nblk > 1) {   // one tile has no edge to merge across
    hipLaunchKernelGGL(cc_merge_kernel, dim3((unsigned)vu_cdiv64(N, 256)), dim3(256), 0, st, labels, ovf, H, W, N, conn, cap);
    snprintf(what, sizeof what, "%s/merge", who);
    rc = vu_check_launch(what);
    if (rc) return rc;
    hipLaunchKernelGGL(cc_compress_kernel, dim3((unsigned)vu_cdiv64(N, 256)), dim3(256), 0, st, labels, ovf, N, cap);
    snprintf(what, sizeof what, "%s/compress", who);
    rc = vu_check_launch(what);
    if (rc) return rc;
  }
  hipLaunchKernelGGL(cc_flatten_kernel, dim3((unsigned)nblk), dim3(256), 0, st, labels, sizes, ovf, D, H, W, tiles_y, tiles_x, conn3,
                     want_flags, cap, vec_lab);
  snprintf(what, sizeof what, "%s/flatten", who);
  return vu_check_launch(what);
}

// scratch of vu_seg_clean: labels | sizes | acc (D,4) uint64 | overflow word (16 bytes) | partial counts
struct clean_layout { size_t labels, sizes, acc, ovf, partials, total; };
clean_layout make_layout(int D, int H, int W) {
  const size_t N = (size_t)D * H * W;
  clean_layout l;
  l.labels = 0;
  l.sizes = vu_align_up(l.labels + N * 4, 16);
  l.acc = vu_align_up(l.sizes + N * 4, 16);
  l.ovf = l.acc + (size_t)D * 32;
  l.partials = l.ovf + 16;
  l.total = l.partials + (size_t)D * (size_t)blocks_per_slice(H, W) * 3 * sizeof(uint32_t);
  return l;
}

}  // namespace

extern "C" {

int vu_cc_tile(int* th, int* tw) {
  VU_REQUIRE(th && tw, "cc_tile: null argument");
  *th = TH;
  *tw = TW;
  return VU_OK;
}

size_t vu_cc_scratch_bytes(int D, int H, int W) {
  if (D <= 0 || H <= 0 || W <= 0) return 0;
  return 16;   // the overflow word
}

int vu_cc_label(const uint8_t* mask, int32_t* labels, uint32_t* sizes, void* scratch, size_t scratch_bytes, int D, int H, int W,
                int conn, int fg, void* stream) {
  int rc = check_shape("cc_label", D, H, W, conn);
  if (rc) return rc;
  VU_REQUIRE(fg == 0 || fg == 1, "cc_label: fg must be 1 (label mask != 0) or 0 (label mask == 0) (got %d)", fg);
  VU_REQUIRE(mask && labels && scratch, "cc_label: null argument (mask, labels and scratch are required)");
  const size_t N = (size_t)D * H * W, need = vu_cc_scratch_bytes(D, H, W);
  VU_REQUIRE(scratch_bytes >= need && aligned_to(scratch, 4), "cc_label: scratch too small or misaligned (%zu bytes needed)", need);
  VU_REQUIRE(aligned_to(labels, 4) && aligned_to(sizes, 4), "cc_label: labels and sizes must be 4-byte aligned");
  VU_REQUIRE(!ranges_overlap(mask, N, labels, N * 4) && !(sizes && ranges_overlap(mask, N, sizes, N * 4)) &&
                 !(sizes && ranges_overlap(labels, N * 4, sizes, N * 4)) && !ranges_overlap(scratch, need, labels, N * 4) &&
                 !ranges_overlap(scratch, need, mask, N) && !(sizes && ranges_overlap(scratch, need, sizes, N * 4)),
             "cc_label: mask, labels, sizes and scratch must not overlap");
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(scratch, 0, need, st) != hipSuccess) {
    vu_set_error("cc_label: clearing the scratch failed: %s", hipGetErrorString(hipGetLastError()));
    return VU_ELAUNCH;
  }
  return label_launch("vu_cc_label", mask, labels, sizes, (unsigned*)scratch, D, H, W, conn, fg, 0, st);
}

size_t vu_seg_clean_scratch_bytes(int D, int H, int W) {
  if (D <= 0 || H <= 0 || W <= 0 || (long long)D * H * W > 0x7fffffffLL) return 0;
  return make_layout(D, H, W).total;
}

int vu_seg_clean(const uint8_t* mask, const uint8_t* truth, uint8_t* out, unsigned long long* counts, long long* stats, void* scratch,
                 size_t scratch_bytes, int D, int H, int W, int conn, unsigned min_size, int keep_largest, int fill_holes, int label,
                 void* stream) {
  int rc = check_shape("seg_clean", D, H, W, conn);
  if (rc) return rc;
  VU_REQUIRE(label <= 255, "seg_clean: label must be negative (any non-zero truth) or 0 .. 255 (got %d)", label);
  VU_REQUIRE((keep_largest == 0 || keep_largest == 1) && (fill_holes == 0 || fill_holes == 1),
             "seg_clean: keep_largest and fill_holes are 0 or 1 (got %d, %d)", keep_largest, fill_holes);
  VU_REQUIRE(mask && out && scratch, "seg_clean: null argument (mask, out and scratch are required)");
  VU_REQUIRE(!truth == !counts, "seg_clean: truth and counts go together (counts need a truth volume, a truth needs counts)");
  const size_t N = (size_t)D * H * W;
  const clean_layout lay = make_layout(D, H, W);
  VU_REQUIRE(scratch_bytes >= lay.total && aligned_to(scratch, 16), "seg_clean: scratch too small or misaligned (%zu bytes needed, 16-byte aligned)",
             lay.total);
  VU_REQUIRE(aligned_to(counts, 8) && aligned_to(stats, 8), "seg_clean: counts and stats must be 8-byte aligned");
  const bool conn3 = conn == 6 || conn == 26;
  const int U = conn3 ? 1 : D;
  VU_REQUIRE(out == mask || !ranges_overlap(mask, N, out, N), "seg_clean: out is the mask itself or does not overlap it");
  VU_REQUIRE(!ranges_overlap(scratch, lay.total, mask, N) && !ranges_overlap(scratch, lay.total, out, N) &&
                 !(truth && ranges_overlap(scratch, lay.total, truth, N)) && !(truth && ranges_overlap(out, N, truth, N)) &&
                 !(counts && ranges_overlap(scratch, lay.total, counts, (size_t)D * 24)) &&
                 !(stats && ranges_overlap(scratch, lay.total, stats, (size_t)U * 32)) &&
                 !(counts && ranges_overlap(out, N, counts, (size_t)D * 24)) && !(stats && ranges_overlap(out, N, stats, (size_t)U * 32)),
             "seg_clean: the scratch and the outputs must not overlap each other, the mask or the truth");
  const long long nb = blocks_per_slice(H, W), per_slice = (long long)H * ((W + 3) / 4);
  const long long unit_px = conn3 ? (long long)N : (long long)H * W, bpu = vu_cdiv64(unit_px, 1024);
  VU_REQUIRE(nb * D <= 0x7fffffffLL && bpu * U <= 0x7fffffffLL, "seg_clean: launch too large (%d slices of %d x %d)", D, H, W);

  hipStream_t st = (hipStream_t)stream;
  char* base = (char*)scratch;
  int* labels = (int*)(base + lay.labels);
  uint32_t* sizes = (uint32_t*)(base + lay.sizes);
  unsigned long long* acc = (unsigned long long*)(base + lay.acc);
  unsigned* ovf = (unsigned*)(base + lay.ovf);
  uint32_t* partials = counts ? (uint32_t*)(base + lay.partials) : (uint32_t*)nullptr;
  if (hipMemsetAsync(acc, 0, lay.partials - lay.acc, st) != hipSuccess) {
    vu_set_error("seg_clean: clearing the scratch failed: %s", hipGetErrorString(hipGetLastError()));
    return VU_ELAUNCH;
  }
  rc = label_launch("vu_seg_clean/label", mask, labels, sizes, ovf, D, H, W, conn, 1, 0, st);
  if (rc) return rc;
  hipLaunchKernelGGL(clean_select_kernel, dim3((unsigned)(bpu * U)), dim3(256), 0, st, (const uint32_t*)sizes, acc, unit_px, (int)bpu,
                     min_size);
  rc = vu_check_launch("vu_seg_clean/select");
  if (rc) return rc;
  const int vec = W % 4 == 0 ? 1 : 0;
  const int vec_out = (vec && aligned_to(out, 4)) ? 1 : 0, vec_truth = (vec && truth && aligned_to(truth, 4)) ? 1 : 0;
  const dim3 grid((unsigned)(nb * D));
  hipLaunchKernelGGL(clean_write_kernel<0>, grid, dim3(256), 0, st, (const int*)labels, (const uint32_t*)sizes,
                     (const unsigned long long*)acc, (const uint8_t*)nullptr, truth, out, fill_holes ? (uint32_t*)nullptr : partials, H, W,
                     (int)nb, (int)per_slice, conn3 ? 1 : 0, min_size, keep_largest, label, vec, vec_out, vec_truth);
  rc = vu_check_launch("vu_seg_clean/write");
  if (rc) return rc;
  if (fill_holes) {
    rc = label_launch("vu_seg_clean/holes", out, labels, sizes, ovf, D, H, W, dual_conn(conn), 0, 1, st);
    if (rc) return rc;
    hipLaunchKernelGGL(clean_write_kernel<1>, grid, dim3(256), 0, st, (const int*)labels, (const uint32_t*)sizes,
                       (const unsigned long long*)acc, (const uint8_t*)out, truth, out, partials, H, W, (int)nb, (int)per_slice,
                       conn3 ? 1 : 0, min_size, keep_largest, label, vec, vec_out, vec_truth);
    rc = vu_check_launch("vu_seg_clean/fill");
    if (rc) return rc;
  }
  if (counts) {
    hipLaunchKernelGGL(clean_counts_kernel, dim3(D), dim3(256), 0, st, (const uint32_t*)partials, counts, (int)nb);
    rc = vu_check_launch("vu_seg_clean/counts");
    if (rc) return rc;
  }
  if (stats) {
    hipLaunchKernelGGL(clean_stats_kernel, dim3((unsigned)vu_cdiv(U, 256)), dim3(256), 0, st, (const unsigned long long*)acc,
                       (const unsigned*)ovf, stats, U, min_size, keep_largest);
    rc = vu_check_launch("vu_seg_clean/stats");
  }
  return rc;
}

}  // extern "C"
