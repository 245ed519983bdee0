// Guidance energy + its gradient w.r.t. the current activations (losses.py:4-84), on
// channels-last maps [cell][C] so that a cell gather is one coalesced row read.
//
//   fg term   = mean_c mean_n | A1[c, o_n] - A2[c, t_n] |          (pairs, duplicates kept)
//   bg global = mean_c | mean_{BGo} F1[c] - mean_{BGt} F2[c] |
//   bg local  = fg-style term over the identity pairs of BG_both
//   A = pool_p(w F) / (pool_p(w) + 1e-10), w = indicator of the cells named by the index lists
//
// The gradient is accumulated per target cell from a CSR (target cell -> source cells)
// built by a counting sort: every output element has exactly one writer, sign sums are
// integers, so the gradient is bit-deterministic with no float atomics.  Loss values are
// accumulated in float64 (segment order is the only order dependence).
#include "common.h"

#include <cmath>

namespace dh {

// ---- map load / store (with optional bilinear resize, align_corners = False) ----------
__device__ __forceinline__ void bilinear_src(int dst, int n_in, float scale, int& i0, int& i1, float& l0, float& l1) {
  float s = scale * ((float)dst + 0.5f) - 0.5f;
  if (s < 0.f) s = 0.f;
  i0 = (int)s;
  if (i0 > n_in - 1) i0 = n_in - 1;
  i1 = i0 + (i0 < n_in - 1 ? 1 : 0);
  l1 = s - (float)i0;
  l0 = 1.f - l1;
}

template <class T>
__global__ void k_load_map(const T* src, float* dst, int C, int hin, int win, int grid) {
  const int cell = blockIdx.x;
  const int y = cell / grid, x = cell - y * grid;
  if (hin == grid && win == grid) {
    for (int c = threadIdx.x; c < C; c += blockDim.x) dst[(size_t)cell * C + c] = to_f32<T>(src[(size_t)cell * C + c]);
    return;
  }
  int y0, y1, x0, x1;
  float ly0, ly1, lx0, lx1;
  bilinear_src(y, hin, (float)hin / (float)grid, y0, y1, ly0, ly1);
  bilinear_src(x, win, (float)win / (float)grid, x0, x1, lx0, lx1);
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    float v00 = to_f32<T>(src[((size_t)y0 * win + x0) * C + c]);
    float v01 = to_f32<T>(src[((size_t)y0 * win + x1) * C + c]);
    float v10 = to_f32<T>(src[((size_t)y1 * win + x0) * C + c]);
    float v11 = to_f32<T>(src[((size_t)y1 * win + x1) * C + c]);
    dst[(size_t)cell * C + c] = ly0 * (lx0 * v00 + lx1 * v01) + ly1 * (lx0 * v10 + lx1 * v11);
  }
}

// transpose of k_load_map: one block per INPUT cell, gathers from the grid cells that read it.
// The gather window, per axis.  Grid row y reads input rows i0 = floor(s) and i0 + 1 at s = sy (y + 0.5) - 0.5, so it
// reads row yi with a non-zero weight only if yi - 1 < s < yi + 1, that is
//     (yi - 0.5) / sy - 0.5  <  y  <  (yi + 1.5) / sy - 0.5        (sy = h_in / grid, any ratio)
// The two clamps of bilinear_src stay inside it: s < 0 becomes s = 0 and reads row 0 alone -- those y lie below the upper
// bound of yi = 0 and the window's lower end is clamped to 0; i0 = n_in - 1 reads the last row alone (i1 = i0) -- those y
// have s >= n_in - 1 > yi - 1 for yi = n_in - 1 and the upper end is clamped to grid - 1.  One more cell on either side
// absorbs the f32 rounding of the bounds; a cell of the window that does not read (yi, xi) has weight 0 and is skipped,
// so the cells that count are added in ascending (y, x) order whatever the window's width.
template <class T>
__global__ void k_store_grad(const float* g, T* out, int C, int hin, int win, int grid, float scale) {
  const int cell = blockIdx.x;
  if (hin == grid && win == grid) {
    for (int c = threadIdx.x; c < C; c += blockDim.x)
      out[(size_t)cell * C + c] = from_f32<T>(g[(size_t)cell * C + c] * scale);
    return;
  }
  const int yi = cell / win, xi = cell - yi * win;
  const float sy = (float)hin / (float)grid, sx = (float)win / (float)grid;
  int ylo = (int)floorf(((float)yi - 0.5f) / sy - 0.5f) - 1, yhi = (int)ceilf(((float)yi + 1.5f) / sy - 0.5f) + 1;
  int xlo = (int)floorf(((float)xi - 0.5f) / sx - 0.5f) - 1, xhi = (int)ceilf(((float)xi + 1.5f) / sx - 0.5f) + 1;
  ylo = ylo < 0 ? 0 : ylo; xlo = xlo < 0 ? 0 : xlo;
  yhi = yhi > grid - 1 ? grid - 1 : yhi; xhi = xhi > grid - 1 ? grid - 1 : xhi;
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    float acc = 0.f;
    for (int y = ylo; y <= yhi; ++y) {
      int y0, y1; float ly0, ly1;
      bilinear_src(y, hin, sy, y0, y1, ly0, ly1);
      float wy = (y0 == yi ? ly0 : 0.f) + (y1 == yi ? ly1 : 0.f);
      if (wy == 0.f) continue;
      for (int x = xlo; x <= xhi; ++x) {
        int x0, x1; float lx0, lx1;
        bilinear_src(x, win, sx, x0, x1, lx0, lx1);
        float wx = (x0 == xi ? lx0 : 0.f) + (x1 == xi ? lx1 : 0.f);
        if (wx == 0.f) continue;
        acc += wy * wx * g[((size_t)y * grid + x) * C + c];
      }
    }
    out[(size_t)cell * C + c] = from_f32<T>(acc * scale);
  }
}

// ---- CSR: target cell -> list of source cells -----------------------------------------
__global__ void k_hist(const int* pairs, int n, int* cnt, uint8_t* w1, uint8_t* w2) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int o = pairs[2 * (size_t)i], t = pairs[2 * (size_t)i + 1];
  atomicAdd(&cnt[t], 1);
  w1[o] = 1;
  w2[t] = 1;
}

__global__ void k_identity_pairs(const int* list, int n, int* pairs) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  pairs[2 * (size_t)i] = list[i];
  pairs[2 * (size_t)i + 1] = list[i];
}

// exclusive scan of cnt[0..n) into off[0..n], cursor copy; single workgroup of 1024
__global__ void __launch_bounds__(1024) k_scan_cells(const int* cnt, int n, int* off, int* cursor) {
  __shared__ int sm[1024];
  __shared__ int carry;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (int base = 0; base < n; base += 1024) {
    int i = base + threadIdx.x;
    int v = i < n ? cnt[i] : 0;
    sm[threadIdx.x] = v;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
      int t = threadIdx.x >= o ? sm[threadIdx.x - o] : 0;
      __syncthreads();
      sm[threadIdx.x] += t;
      __syncthreads();
    }
    int excl = sm[threadIdx.x] - v + carry;
    if (i < n) { off[i] = excl; cursor[i] = excl; }
    __syncthreads();
    if (threadIdx.x == 1023) carry += sm[1023];
    __syncthreads();
  }
  if (threadIdx.x == 0) off[n] = carry;
}

__global__ void k_fill(const int* pairs, int n, int* cursor, int* src) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int o = pairs[2 * (size_t)i], t = pairs[2 * (size_t)i + 1];
  src[atomicAdd(&cursor[t], 1)] = o;
}

// ---- pooling --------------------------------------------------------------------------
// out[cell][c] = sum_window(w * X) / (sum_window(w) + p*p*1e-10); den[cell] = that denominator
__global__ void k_pool(const float* X, const uint8_t* w, int C, int grid, int p, float* out, float* den) {
  const int cell = blockIdx.x, y = cell / grid, x = cell - y * grid, r = p / 2;
  float wn = 0.f;
  for (int dy = -r; dy <= r; ++dy)
    for (int dx = -r; dx <= r; ++dx) {
      int yy = y + dy, xx = x + dx;
      if (yy >= 0 && yy < grid && xx >= 0 && xx < grid && w[yy * grid + xx]) wn += 1.f;
    }
  const float d = wn + (float)(p * p) * 1e-10f;
  if (threadIdx.x == 0) den[cell] = d;
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    float s = 0.f;
    for (int dy = -r; dy <= r; ++dy)
      for (int dx = -r; dx <= r; ++dx) {
        int yy = y + dy, xx = x + dx;
        if (yy >= 0 && yy < grid && xx >= 0 && xx < grid && w[yy * grid + xx]) s += X[((size_t)yy * grid + xx) * C + c];
      }
    out[(size_t)cell * C + c] = s / d;
  }
}

// acc[cell][c] += w[cell] * sum_window(G / den)
__global__ void k_spread(const float* G, const uint8_t* w, const float* den, int C, int grid, int p, float* acc) {
  const int cell = blockIdx.x, y = cell / grid, x = cell - y * grid, r = p / 2;
  if (!w[cell]) return;
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    float s = 0.f;
    for (int dy = -r; dy <= r; ++dy)
      for (int dx = -r; dx <= r; ++dx) {
        int yy = y + dy, xx = x + dx;
        if (yy >= 0 && yy < grid && xx >= 0 && xx < grid) s += G[((size_t)yy * grid + xx) * C + c] / den[yy * grid + xx];
      }
    acc[(size_t)cell * C + c] += s;
  }
}

// ---- pair term --------------------------------------------------------------------------
// one block per target cell t: G[t][c] (+)= -coef * sum_{k in seg(t)} sign(X1[src_k][c] - X2[t][c])
__global__ void k_pair_term(const float* X1, const float* X2, const int* off, const int* src, int C, float coef,
                            float* G, int accumulate, double* loss_part) {
  __shared__ double sm[4];
  const int t = blockIdx.x;
  const int b = off[t], e = off[t + 1];
  double l = 0.0;
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    const float a = X2[(size_t)t * C + c];
    int s = 0;
    double la = 0.0;
    for (int k = b; k < e; ++k) {
      float d = X1[(size_t)src[k] * C + c] - a;
      la += (double)fabsf(d);
      s += (d > 0.f) - (d < 0.f);
    }
    float g = -coef * (float)s;
    if (accumulate) G[(size_t)t * C + c] += g; else G[(size_t)t * C + c] = g;
    l += la;
  }
  l = block_sum(l, sm);
  if (threadIdx.x == 0) loss_part[t] = l;
}

// ---- global-average term ----------------------------------------------------------------
// part[s][c] = sum over the s-th slice of `list` of X[cell][c]
__global__ void k_colsum(const float* X, const int* list, int n, int C, int S, float* part) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x, s = blockIdx.y;
  if (c >= C) return;
  const int per = (n + S - 1) / S, b = s * per, e = b + per < n ? b + per : n;
  float acc = 0.f;
  for (int k = b; k < e; ++k) acc += X[(size_t)list[k] * C + c];
  part[(size_t)s * C + c] = acc;
}

// sgn[c] = sign(m1 - m2), loss_c = |m1 - m2|.  Workgroup = 64 channels x 4 waves: wave q adds the slice partials of
// quarter q in slice order, the four quarter sums are added in quarter order (fixed tree: deterministic)
constexpr int GD_BLOCK = 64;
__global__ void __launch_bounds__(4 * GD_BLOCK) k_global_diff(const float* p1, const float* p2, int S, int C, int n1, int n2,
                                                              float* sgn, double* loss_part) {
  __shared__ float sq[2][4][GD_BLOCK];
  const int cl = threadIdx.x & (GD_BLOCK - 1), q = threadIdx.x / GD_BLOCK;
  const int c = blockIdx.x * GD_BLOCK + cl;
  const int per = (S + 3) / 4, s0 = q * per, s1 = s0 + per < S ? s0 + per : S;
  float a = 0.f, b = 0.f;
  if (c < C) {
    int s = s0;
    for (; s + 8 <= s1; s += 8) {
      float va[8], vb[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) { va[j] = p1[(size_t)(s + j) * C + c]; vb[j] = p2[(size_t)(s + j) * C + c]; }
#pragma unroll
      for (int j = 0; j < 8; ++j) { a += va[j]; b += vb[j]; }
    }
    for (; s < s1; ++s) { a += p1[(size_t)s * C + c]; b += p2[(size_t)s * C + c]; }
  }
  sq[0][q][cl] = a; sq[1][q][cl] = b;
  __syncthreads();
  if (q != 0) return;
  double l = 0.0;
  if (c < C) {
    a = ((sq[0][0][cl] + sq[0][1][cl]) + sq[0][2][cl]) + sq[0][3][cl];
    b = ((sq[1][0][cl] + sq[1][1][cl]) + sq[1][2][cl]) + sq[1][3][cl];
    const float d = a / (float)n1 - b / (float)n2;
    sgn[c] = (float)((d > 0.f) - (d < 0.f));
    l = (double)fabsf(d);
  }
  l = wave_sum(l);
  if (threadIdx.x == 0) loss_part[blockIdx.x] = l;
}

__global__ void k_global_apply(const int* list, int n, const float* sgn, int C, float coef, float* acc) {
  const int cell = list[blockIdx.x];
  for (int c = threadIdx.x; c < C; c += blockDim.x) acc[(size_t)cell * C + c] += -coef * sgn[c];
}

__global__ void k_final_loss(const double* fg_part, int n_fg_part, float fg_norm, const double* bg_part, int n_bg_part,
                             float bg_norm, float fg_w, float bg_w, float* out) {
  __shared__ double sm[4];
  double a = 0.0, b = 0.0;
  for (int i = threadIdx.x; i < n_fg_part; i += blockDim.x) a += fg_part[i];
  for (int i = threadIdx.x; i < n_bg_part; i += blockDim.x) b += bg_part[i];
  a = block_sum(a, sm);
  b = block_sum(b, sm);
  if (threadIdx.x == 0) {
    float fg = (float)(a * (double)fg_norm), bg = (float)(b * (double)bg_norm);
    out[0] = fg_w * fg + bg_w * bg;
    out[1] = fg;
    out[2] = bg;
  }
}

struct EnergyWs {
  float *cur, *orig, *acc, *A1, *A2, *G, *den1, *den2, *part1, *part2, *sgn;
  int *cnt, *off, *cursor, *src, *idpairs;
  uint8_t *w1, *w2;
  double *fg_part, *bg_part;
};
constexpr int COLSUM_S = 128;     // slices of a background column sum (more slices = shorter serial gather chains)

static bool carve_energy(Arena& a, int C, int grid, int n_pairs, EnergyWs& w) {
  const size_t G2 = (size_t)grid * grid, M = G2 * C;
  const size_t np = (size_t)(n_pairs > (int)G2 ? n_pairs : (int)G2);
  w.cur = a.take<float>(M); w.orig = a.take<float>(M); w.acc = a.take<float>(M);
  w.A1 = a.take<float>(M); w.A2 = a.take<float>(M); w.G = a.take<float>(M);
  w.den1 = a.take<float>(G2); w.den2 = a.take<float>(G2);
  w.part1 = a.take<float>((size_t)COLSUM_S * C); w.part2 = a.take<float>((size_t)COLSUM_S * C);
  w.sgn = a.take<float>(C);
  w.cnt = a.take<int>(G2 + 1); w.off = a.take<int>(G2 + 1); w.cursor = a.take<int>(G2 + 1);
  w.src = a.take<int>(np); w.idpairs = a.take<int>(2 * G2);
  w.w1 = a.take<uint8_t>(G2); w.w2 = a.take<uint8_t>(G2);
  w.fg_part = a.take<double>(G2); w.bg_part = a.take<double>(G2);
  return a.ok();
}

template <class T>
static void launch_load(const void* src, float* dst, int C, int hin, int win, int grid, hipStream_t st) {
  hipLaunchKernelGGL((k_load_map<T>), dim3(grid * grid), dim3(256), 0, st, (const T*)src, dst, C, hin, win, grid);
}
template <class T>
static void launch_store(const float* g, void* out, int C, int hin, int win, int grid, float scale, hipStream_t st) {
  hipLaunchKernelGGL((k_store_grad<T>), dim3(hin * win), dim3(256), 0, st, g, (T*)out, C, hin, win, grid, scale);
}

// one pair-type term: CSR build, optional pooling, gradient into acc, loss partials into part
static void pair_term(const EnergyWs& w, const int* pairs, int n, int C, int grid, int patch, float coef,
                      double* part, hipStream_t st) {
  const int G2 = grid * grid;
  (void)hipMemsetAsync(w.cnt, 0, (G2 + 1) * sizeof(int), st);
  (void)hipMemsetAsync(w.w1, 0, G2, st);
  (void)hipMemsetAsync(w.w2, 0, G2, st);
  hipLaunchKernelGGL(k_hist, dim3(cdiv(n, 256)), dim3(256), 0, st, pairs, n, w.cnt, w.w1, w.w2);
  hipLaunchKernelGGL(k_scan_cells, dim3(1), dim3(1024), 0, st, w.cnt, G2, w.off, w.cursor);
  hipLaunchKernelGGL(k_fill, dim3(cdiv(n, 256)), dim3(256), 0, st, pairs, n, w.cursor, w.src);
  if (patch <= 1) {
    hipLaunchKernelGGL(k_pair_term, dim3(G2), dim3(256), 0, st, w.orig, w.cur, w.off, w.src, C, coef, w.acc, 1, part);
  } else {
    hipLaunchKernelGGL(k_pool, dim3(G2), dim3(256), 0, st, w.orig, w.w1, C, grid, patch, w.A1, w.den1);
    hipLaunchKernelGGL(k_pool, dim3(G2), dim3(256), 0, st, w.cur, w.w2, C, grid, patch, w.A2, w.den2);
    hipLaunchKernelGGL(k_pair_term, dim3(G2), dim3(256), 0, st, w.A1, w.A2, w.off, w.src, C, coef, w.G, 0, part);
    hipLaunchKernelGGL(k_spread, dim3(G2), dim3(256), 0, st, w.G, w.w2, w.den2, C, grid, patch, w.acc);
  }
}

// ---- planned fast path ------------------------------------------------------------------
// The default configuration (maps already at the cell grid, fg_patch 1, 'global_avg' background) needs no f32
// staging, no pooling and -- because the correspondences are fixed for an edit -- no CSR rebuild per evaluation:
//   plan (once per edit)  : CSR target cell -> source cells, flag of the transformed-background cells
//   per evaluation        : k_colsum_q (both background column sums in the slice order of k_colsum, combined per quarter of
//                                       the slices as k_global_diff combines them)
//                           k_energy_grad (prologue: sign of the mean difference per channel from the quarter sums -- the rest of
//                                          k_global_diff's arithmetic; then pair term + background term -> one 16-byte gradient store per lane)
//                           k_final_loss  (only when the caller wants the loss values)
// Same arithmetic, in the same order per element, as the general path above: the gradient is bit-identical.
struct EnergyPlan {
  int *off, *src, *cnt, *cursor, *mult;      // after the build: cnt[t] = number of DISTINCT sources of target t,
  uint8_t *bgflag, *w1, *w2;                 // src / mult [off[t], off[t] + cnt[t]) = their cells (ascending) / multiplicities
};
static bool carve_plan(Arena& a, int grid, int n_pairs, EnergyPlan& p) {
  const size_t G2 = (size_t)grid * grid;
  p.off = a.take<int>(G2 + 1); p.cnt = a.take<int>(G2 + 1); p.cursor = a.take<int>(G2 + 1);
  p.src = a.take<int>(n_pairs > 0 ? n_pairs : 1);
  p.mult = a.take<int>(n_pairs > 0 ? n_pairs : 1);
  p.bgflag = a.take<uint8_t>(G2); p.w1 = a.take<uint8_t>(G2); p.w2 = a.take<uint8_t>(G2);
  return a.ok();
}
struct PlannedWs {
  float* partq;                  // [2 lists][4 quarters][C] quarter sums of the background column sums (k_colsum_q)
  double *fg_part, *bg_part;
};
static bool carve_planned(Arena& a, int C, int grid, PlannedWs& w) {
  const size_t G2 = (size_t)grid * grid;
  w.partq = a.take<float>((size_t)8 * C);
  w.fg_part = a.take<double>(G2); w.bg_part = a.take<double>(2);
  return a.ok();
}

// The distinct cells of the workgroup's LDS histogram, in ascending order, with their counts -> src / mult [pos0 ..), and m -> obj
// there when the plan keeps an object per entry.  Returns how many, in every thread, behind a barrier: hist and scan are free.
__device__ __forceinline__ int emit_distinct(const int* hist, int* scan, int G2, int pos0, int* src, int* mult, uint8_t* obj, int m) {
  const int per = (G2 + blockDim.x - 1) / blockDim.x, c0 = threadIdx.x * per, c1 = min(c0 + per, G2);
  int mine = 0;
  for (int c = c0; c < c1; ++c) mine += hist[c] != 0;
  scan[threadIdx.x] = mine;
  __syncthreads();
  for (int o = 1; o < (int)blockDim.x; o <<= 1) {
    const int v = (int)threadIdx.x >= o ? scan[threadIdx.x - o] : 0;
    __syncthreads();
    scan[threadIdx.x] += v;
    __syncthreads();
  }
  int pos = pos0 + scan[threadIdx.x] - mine;
  for (int c = c0; c < c1; ++c)
    if (hist[c]) {
      src[pos] = c; mult[pos] = hist[c];
      if (obj) obj[pos] = (uint8_t)m;
      ++pos;
    }
  const int n = scan[blockDim.x - 1];
  __syncthreads();
  return n;
}

// one workgroup per target cell: its source list (one entry per pixel pair: ~8x8 pixels share a cell pair) becomes
// (distinct source cell, multiplicity) in ascending cell order, through an LDS histogram over the grid's cells
__global__ void __launch_bounds__(256) k_dedupe_sources(const int* off, int* src, int* mult, int* ucnt, int G2) {
  extern __shared__ int hist[];          // [G2] counts, then [256] scan scratch
  const int t = blockIdx.x, b = off[t], e = off[t + 1];
  if (b == e) { if (threadIdx.x == 0) ucnt[t] = 0; return; }
  for (int c = threadIdx.x; c < G2; c += blockDim.x) hist[c] = 0;
  __syncthreads();
  for (int k = b + threadIdx.x; k < e; k += blockDim.x) atomicAdd(&hist[src[k]], 1);
  __syncthreads();
  const int n = emit_distinct(hist, hist + G2, G2, b, src, mult, nullptr, 0);
  if (threadIdx.x == 0) ucnt[t] = n;
}

__global__ void k_flag_cells(const int* list, int n, uint8_t* flag) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) flag[list[i]] = 1;
}

// Background (global_avg) term, first half (round 5: the evaluation is two launches, k_colsum_q -> k_energy_grad; it used to be
// k_colsum16 -> k_global_diff -> k_energy_grad).  Workgroup = (64 channels, quarter q of the COLSUM_S = 128 slices, list z); thread
// = (slice of the quarter, 8-channel chunk): the eight lanes of a slice read 128 contiguous bytes of a row.  A thread adds the rows
// of its slice in list order (16 gathers in flight), the 32 slice sums of the quarter are added in slice order through LDS:
// partq[z][q][c] -- exactly k_colsum's slices combined the way k_global_diff combines the slices of a quarter, so that
// ((q0 + q1) + q2) + q3 in k_energy_grad's prologue reproduces sgn[c] bit for bit.
constexpr int CQ_SL = COLSUM_S / 4;          // slices per quarter
template <class T>
__global__ void __launch_bounds__(8 * CQ_SL) k_colsum_q(const T* X1, const int* list1, int n1, const T* X2, const int* list2, int n2,
                                                       int C, float* partq) {
  const int z = blockIdx.z;
  const T* X = z ? X2 : X1;
  const int* list = z ? list2 : list1;
  const int n = z ? n2 : n1;
#include "colsum_q_body.inc"
}

// thread = (target cell, 8-channel chunk); block = 256 / (C/8) cells
template <class T, class TG>
__global__ void __launch_bounds__(256) k_energy_grad(const T* orig, const T* cur, const int* off, const int* ucnt,
                                                     const int* src, const int* mult, const uint8_t* bgflag, const float* partq, int n1, int n2,
                                                     int C, int G2, float coef_fg,
                                                     float coef_bg, int use_bg, float scale, TG* grad, double* loss_part, double* bg_loss) {
#include "energy_grad_body.inc"
}

// ---- K items in one launch pair (dh_energy_fwd_bwd_planned_batch) ---------------------------------------------------------
// Everything an item's kernels need, carved and derived on the host; the table travels BY VALUE in the kernel arguments
// (16 x 160 B: no device allocation, no copy, no synchronisation on the step path) and a workgroup reads its item's row
// through scalar loads (the item index is a block index).  The bodies are the single kernels' own text.
constexpr int ENERGY_MAX_ITEMS = 16;
struct EnergyItem {
  const void *orig, *cur;
  const int *off, *ucnt, *src, *mult;
  const uint8_t* bgflag;
  const int *list1, *list2;
  float* partq;
  void* grad;
  double *loss_part, *bg_loss;
  float* loss_out;
  int n1, n2, use_bg, n_fg_part;
  float coef_fg, coef_bg, scale, fg_norm, bg_norm, fg_w, bg_w;
};
struct EnergyBatch {
  EnergyItem it[ENERGY_MAX_ITEMS];
};

// grid (C / 64, 4 quarters, 2 K): list z & 1 of item z / 2; an item without a background term has no work here
template <class T>
__global__ void __launch_bounds__(8 * CQ_SL) k_colsum_q_batch(const EnergyBatch tab, int C) {
  const EnergyItem& it = tab.it[blockIdx.z >> 1];
  if (!it.use_bg) return;
  const int z = blockIdx.z & 1;
  const T* X = (const T*)(z ? it.cur : it.orig);
  const int* list = z ? it.list2 : it.list1;
  const int n = z ? it.n2 : it.n1;
  float* partq = it.partq;
#include "colsum_q_body.inc"
}

// grid (blocks of cells, K): item blockIdx.y, the cells of blockIdx.x
template <class T, class TG>
__global__ void __launch_bounds__(256) k_energy_grad_batch(const EnergyBatch tab, int C, int G2) {
  const EnergyItem& it = tab.it[blockIdx.y];
  const T *orig = (const T*)it.orig, *cur = (const T*)it.cur;
  const int *off = it.off, *ucnt = it.ucnt, *src = it.src, *mult = it.mult;
  const uint8_t* bgflag = it.bgflag;
  const float* partq = it.partq;
  const int n1 = it.n1, n2 = it.n2, use_bg = it.use_bg;
  const float coef_fg = it.coef_fg, coef_bg = it.coef_bg, scale = it.scale;
  TG* grad = (TG*)it.grad;
  double *loss_part = it.loss_part, *bg_loss = it.bg_loss;
#include "energy_grad_body.inc"
}

// one workgroup per item that asked for its loss values: k_final_loss's sums
__global__ void k_final_loss_batch(const EnergyBatch tab) {
  __shared__ double sm[4];
  const EnergyItem& it = tab.it[blockIdx.x];
  if (!it.loss_out) return;
  double a = 0.0, b = 0.0;
  for (int i = threadIdx.x; i < it.n_fg_part; i += blockDim.x) a += it.loss_part[i];
  for (int i = threadIdx.x; i < it.use_bg; i += blockDim.x) b += it.bg_loss[i];
  a = block_sum(a, sm);
  b = block_sum(b, sm);
  if (threadIdx.x == 0) {
    float fg = (float)(a * (double)it.fg_norm), bg = (float)(b * (double)it.bg_norm);
    it.loss_out[0] = it.fg_w * fg + it.bg_w * bg;
    it.loss_out[1] = fg;
    it.loss_out[2] = bg;
  }
}

// ---- a weight per object (dh_energy_plan_build_objects, dh_energy_fwd_bwd_planned_objects[_batch]) --------------------------
// The foreground term becomes sum_m omega_m * mean_c mean_{n in object m} |.|, omega_m = w_m / sum of the weights of the objects
// that have pairs.  The gradient of a target cell then mixes pairs of different objects with different coefficients, so the CSR
// segment of a cell lists distinct (object, source cell) entries in ascending (object, cell) order, with one byte per entry for
// the object.  The plan buffer is carve_plan's, then the raw fill and the object block (layout: energy_grad_obj_body.inc).
constexpr int ENERGY_MAX_OBJECTS = 8;
constexpr int OBJ_HEADER = 128;              // omega[8] f32, N[8] i32, omega / N [8] f64
struct EnergyPlanObj {
  EnergyPlan base;
  int* raw;                                  // the fill before the dedupe: object << 24 | source cell, in the CSR's segments
  uint8_t* objp;                             // header, then the object of every entry of base.src / base.mult
};
static bool carve_plan_obj(Arena& a, int grid, int n_pairs, EnergyPlanObj& p) {
  carve_plan(a, grid, n_pairs, p.base);
  p.raw = a.take<int>(n_pairs > 0 ? n_pairs : 1);
  p.objp = a.take<uint8_t>((size_t)OBJ_HEADER + (n_pairs > 0 ? n_pairs : 1));
  return a.ok();
}
struct ObjHeader {
  float omega[ENERGY_MAX_OBJECTS];
  int n[ENERGY_MAX_OBJECTS];
  double lossw[ENERGY_MAX_OBJECTS];
};
__global__ void k_store_obj_header(const ObjHeader h, uint8_t* objp) {
  const int i = threadIdx.x;
  if (i >= ENERGY_MAX_OBJECTS) return;
  reinterpret_cast<float*>(objp)[i] = h.omega[i];
  reinterpret_cast<int*>(objp + 32)[i] = h.n[i];
  reinterpret_cast<double*>(objp + 64)[i] = h.lossw[i];
}

__global__ void k_fill_obj(const int* pairs, const uint8_t* pair_obj, int n, int* cursor, int* raw) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int o = pairs[2 * (size_t)i], t = pairs[2 * (size_t)i + 1];
  raw[atomicAdd(&cursor[t], 1)] = (int)((unsigned)o | ((unsigned)pair_obj[i] << 24));
}

// k_dedupe_sources per object: M passes over the segment with the one LDS histogram (a G2 x M histogram would not fit); pass m
// appends the distinct source cells of object m in ascending order behind those of the objects before it.  The distinct entries
// of a segment are never more than its raw entries, so every write stays inside the segment.
__global__ void __launch_bounds__(256) k_dedupe_sources_obj(const int* off, const int* raw, int* src, int* mult, uint8_t* obj,
                                                            int* ucnt, int G2, int M) {
  extern __shared__ int hist[];          // [G2] counts, then [256] scan scratch
  const int t = blockIdx.x, b = off[t], e = off[t + 1];
  if (b == e) { if (threadIdx.x == 0) ucnt[t] = 0; return; }
  int base = b;
  for (int m = 0; m < M; ++m) {
    for (int c = threadIdx.x; c < G2; c += blockDim.x) hist[c] = 0;
    __syncthreads();
    for (int k = b + threadIdx.x; k < e; k += blockDim.x) {
      const unsigned key = (unsigned)raw[k];
      const int c = (int)(key & 0xffffffu);
      if ((int)(key >> 24) == m && c < G2) atomicAdd(&hist[c], 1);
    }
    __syncthreads();
    base += emit_distinct(hist, hist + G2, G2, base, src, mult, obj, m);
  }
  if (threadIdx.x == 0) ucnt[t] = base - b;
}

// the source rows of every object are the host image's in these three kernels (energy_grad_obj_body.inc)
#define DH_ENERGY_SRC(m) orig
// k_energy_grad with a weight per object: thread = (target cell, 8-channel chunk); block = 256 / (C/8) cells
template <class T, class TG>
__global__ void __launch_bounds__(256) k_energy_grad_obj(const T* orig, const T* cur, const int* off, const int* ucnt,
                                                         const int* src, const int* mult, const uint8_t* objp, const uint8_t* bgflag,
                                                         const float* partq, int n1, int n2, int C, int G2, float fg_w,
                                                         float coef_bg, int use_bg, float scale, TG* grad, double* loss_part,
                                                         double* bg_loss) {
#include "energy_grad_obj_body.inc"
}

// K items: the item table of the unweighted batch (k_colsum_q_batch and k_final_loss_batch run on it as they are; coef_fg holds
// the plain fg_w) and, next to it, one pointer per item to the object block of its plan -- both by value
struct EnergyObjPtrs {
  const uint8_t* p[ENERGY_MAX_ITEMS];
};
template <class T, class TG>
__global__ void __launch_bounds__(256) k_energy_grad_obj_batch(const EnergyBatch tab, const EnergyObjPtrs ot, int C, int G2) {
  const EnergyItem& it = tab.it[blockIdx.y];
  const T *orig = (const T*)it.orig, *cur = (const T*)it.cur;
  const int *off = it.off, *ucnt = it.ucnt, *src = it.src, *mult = it.mult;
  const uint8_t* objp = ot.p[blockIdx.y];
  const uint8_t* bgflag = it.bgflag;
  const float* partq = it.partq;
  const int n1 = it.n1, n2 = it.n2, use_bg = it.use_bg;
  const float fg_w = it.coef_fg, coef_bg = it.coef_bg, scale = it.scale;
  TG* grad = (TG*)it.grad;
  double *loss_part = it.loss_part, *bg_loss = it.bg_loss;
#include "energy_grad_obj_body.inc"
}

// K items, some weighted and some not, in one launch (dh_energy_fwd_bwd_planned_mixed_batch): ot.p[item] is the object block of
// a weighted item's plan and null for an unweighted one, whose row carries coef_fg = fg_w / (C N) as in k_energy_grad_batch.  The
// branch depends on blockIdx.y alone, so a workgroup is wholly in one arm and the barriers of block_sum are reached by all of
// its threads; each arm is the text of its own kernel, in a scope of its own.
template <class T, class TG>
__global__ void __launch_bounds__(256) k_energy_grad_mixed_batch(const EnergyBatch tab, const EnergyObjPtrs ot, int C, int G2) {
  const EnergyItem& it = tab.it[blockIdx.y];
  const T *orig = (const T*)it.orig, *cur = (const T*)it.cur;
  const int *off = it.off, *ucnt = it.ucnt, *src = it.src, *mult = it.mult;
  const uint8_t* objp = ot.p[blockIdx.y];
  const uint8_t* bgflag = it.bgflag;
  const float* partq = it.partq;
  const int n1 = it.n1, n2 = it.n2, use_bg = it.use_bg;
  const float coef_bg = it.coef_bg, scale = it.scale;
  TG* grad = (TG*)it.grad;
  double *loss_part = it.loss_part, *bg_loss = it.bg_loss;
  if (objp) {
    const float fg_w = it.coef_fg;
#include "energy_grad_obj_body.inc"
  } else {
    const float coef_fg = it.coef_fg;
#include "energy_grad_body.inc"
  }
}
#undef DH_ENERGY_SRC

// ---- donor objects (dh_energy_fwd_bwd_planned_donor[_batch]) ---------------------------------------------------------------
// An object whose bit is set in donor_bits was brought in from another image: the source rows of its pairs are rows of that
// image's activations (donor), not of orig.  The plan, the entries' order and the coefficients are the weighted plan's; only the
// base pointer of an entry's source row is chosen per entry, by a select on the entry's object (both pointers and the bits are
// kernel arguments: scalars).  The background term reads orig, as it always did.
#define DH_ENERGY_SRC(m) (((donor_bits >> (m)) & 1u) ? donor : orig)
template <class T, class TG>
__global__ void __launch_bounds__(256) k_energy_grad_donor(const T* orig, const T* donor, unsigned donor_bits, const T* cur,
                                                           const int* off, const int* ucnt, const int* src, const int* mult,
                                                           const uint8_t* objp, const uint8_t* bgflag, const float* partq, int n1,
                                                           int n2, int C, int G2, float fg_w, float coef_bg, int use_bg,
                                                           float scale, TG* grad, double* loss_part, double* bg_loss) {
#include "energy_grad_obj_body.inc"
}

// K items: the tables of k_energy_grad_obj_batch and, next to them, the donor pointer and the bits of every item -- by value
struct EnergyDonorTab {
  const void* donor[ENERGY_MAX_ITEMS];
  unsigned bits[ENERGY_MAX_ITEMS];
};
template <class T, class TG>
__global__ void __launch_bounds__(256) k_energy_grad_donor_batch(const EnergyBatch tab, const EnergyObjPtrs ot,
                                                                 const EnergyDonorTab dt, int C, int G2) {
  const EnergyItem& it = tab.it[blockIdx.y];
  const T *orig = (const T*)it.orig, *cur = (const T*)it.cur;
  const T* donor = (const T*)dt.donor[blockIdx.y];
  const unsigned donor_bits = dt.bits[blockIdx.y];
  const int *off = it.off, *ucnt = it.ucnt, *src = it.src, *mult = it.mult;
  const uint8_t* objp = ot.p[blockIdx.y];
  const uint8_t* bgflag = it.bgflag;
  const float* partq = it.partq;
  const int n1 = it.n1, n2 = it.n2, use_bg = it.use_bg;
  const float fg_w = it.coef_fg, coef_bg = it.coef_bg, scale = it.scale;
  TG* grad = (TG*)it.grad;
  double *loss_part = it.loss_part, *bg_loss = it.bg_loss;
#include "energy_grad_obj_body.inc"
}
#undef DH_ENERGY_SRC

}  // namespace dh

using namespace dh;

extern "C" int dh_energy_workspace_bytes(int C, int grid, int n_pairs, size_t* bytes) {
  DH_REQUIRE(C >= 1 && grid >= 1 && n_pairs >= 0 && bytes, "bad arguments");
  Arena a(nullptr, (size_t)-1);
  EnergyWs w;
  carve_energy(a, C, grid, n_pairs, w);
  *bytes = a.off + 256;
  return DH_OK;
}

extern "C" int dh_energy_fwd_bwd(const void* cur, const void* orig, int dtype, int C, int h_in, int w_in, int grid,
                                 const int32_t* pairs, int n_pairs, const int32_t* bg_both, int n_bg_both,
                                 const int32_t* bg_orig, int n_bg_orig, const int32_t* bg_trans, int n_bg_trans,
                                 float fg_w, float bg_w, int fg_patch, int bg_patch, int bg_mode, float grad_scale,
                                 float* loss_out, void* grad, int grad_dtype, void* workspace, size_t workspace_bytes,
                                 void* stream) {
  DH_REQUIRE(cur && orig && loss_out && grad && workspace, "null pointer");
  DH_REQUIRE(C >= 1 && h_in >= 1 && w_in >= 1 && grid >= 1, "bad sizes");
  DH_REQUIRE(fg_patch >= 1 && (fg_patch & 1) && bg_patch >= 1 && (bg_patch & 1), "patch sizes must be odd");
  DH_REQUIRE(bg_mode == 0 || bg_mode == 1, "unknown background loss type");
  DH_REQUIRE(dtype >= 0 && dtype <= 2 && grad_dtype >= 0 && grad_dtype <= 2, "bad dtype");
  hipStream_t st = (hipStream_t)stream;
  const int G2 = grid * grid;
  Arena a(workspace, workspace_bytes);
  EnergyWs w;
  DH_REQUIRE(carve_energy(a, C, grid, n_pairs, w), "workspace too small");

  switch (dtype) {
    case DH_DTYPE_F16: launch_load<f16>(cur, w.cur, C, h_in, w_in, grid, st); launch_load<f16>(orig, w.orig, C, h_in, w_in, grid, st); break;
    case DH_DTYPE_BF16: launch_load<bf16>(cur, w.cur, C, h_in, w_in, grid, st); launch_load<bf16>(orig, w.orig, C, h_in, w_in, grid, st); break;
    default: launch_load<float>(cur, w.cur, C, h_in, w_in, grid, st); launch_load<float>(orig, w.orig, C, h_in, w_in, grid, st); break;
  }
  DH_CHECK_HIP(hipMemsetAsync(w.acc, 0, (size_t)G2 * C * sizeof(float), st));
  DH_CHECK_HIP(hipMemsetAsync(w.fg_part, 0, G2 * sizeof(double), st));
  DH_CHECK_HIP(hipMemsetAsync(w.bg_part, 0, G2 * sizeof(double), st));

  float fg_norm = 0.f, bg_norm = 0.f;
  int n_fg_part = 0, n_bg_part = 0;
  if (n_pairs > 0) {   // n == 0 would be NaN in the reference (mean over an empty axis): skipped here
    DH_REQUIRE(pairs, "null pairs");
    fg_norm = 1.f / ((float)C * (float)n_pairs);
    pair_term(w, pairs, n_pairs, C, grid, fg_patch, fg_w * fg_norm, w.fg_part, st);
    n_fg_part = G2;
  }
  if (bg_mode == 0) {
    if (n_bg_orig > 0 && n_bg_trans > 0) {
      DH_REQUIRE(bg_orig && bg_trans, "null bg list");
      hipLaunchKernelGGL(k_colsum, dim3(cdiv(C, 256), COLSUM_S), dim3(256), 0, st, w.orig, bg_orig, n_bg_orig, C,
                         COLSUM_S, w.part1);
      hipLaunchKernelGGL(k_colsum, dim3(cdiv(C, 256), COLSUM_S), dim3(256), 0, st, w.cur, bg_trans, n_bg_trans, C,
                         COLSUM_S, w.part2);
      hipLaunchKernelGGL(k_global_diff, dim3(cdiv(C, GD_BLOCK)), dim3(4 * GD_BLOCK), 0, st, w.part1, w.part2, COLSUM_S, C,
                         n_bg_orig, n_bg_trans, w.sgn, w.bg_part);
      bg_norm = 1.f / (float)C;
      hipLaunchKernelGGL(k_global_apply, dim3(n_bg_trans), dim3(256), 0, st, bg_trans, n_bg_trans, w.sgn, C,
                         bg_w * bg_norm / (float)n_bg_trans, w.acc);
      n_bg_part = cdiv(C, GD_BLOCK);
    }
  } else if (n_bg_both > 0) {
    DH_REQUIRE(bg_both, "null bg list");
    hipLaunchKernelGGL(k_identity_pairs, dim3(cdiv(n_bg_both, 256)), dim3(256), 0, st, bg_both, n_bg_both, w.idpairs);
    bg_norm = 1.f / ((float)C * (float)n_bg_both);
    pair_term(w, w.idpairs, n_bg_both, C, grid, bg_patch, bg_w * bg_norm, w.bg_part, st);
    n_bg_part = G2;
  }
  hipLaunchKernelGGL(k_final_loss, dim3(1), dim3(256), 0, st, w.fg_part, n_fg_part, fg_norm, w.bg_part, n_bg_part,
                     bg_norm, fg_w, bg_w, loss_out);
  switch (grad_dtype) {
    case DH_DTYPE_F16: launch_store<f16>(w.acc, grad, C, h_in, w_in, grid, grad_scale, st); break;
    case DH_DTYPE_BF16: launch_store<bf16>(w.acc, grad, C, h_in, w_in, grid, grad_scale, st); break;
    default: launch_store<float>(w.acc, grad, C, h_in, w_in, grid, grad_scale, st); break;
  }
  DH_LAUNCH_CHECK();
  return DH_OK;
}

// ---- planned path, host side ------------------------------------------------------------------------------------------------
// One routine per job, whatever the entry: build_plan (both plan builds), fill_item (every derived constant of an item, for
// single and batched calls alike -- item e of a batch is bit-identical to its single call because both rows come from here),
// run_planned_single and run_planned_batch (the launches).  `who` is the entry's name: error texts name the entry, not a helper.
static int refuse(const char* who, const char* msg) {
  set_error(std::string(who) + ": " + msg);
  return DH_ERR_ARG;
}
static int launch_status(const char* who) {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return DH_OK;
  set_error(std::string(who) + " launch: " + hipGetErrorString(e));
  return DH_ERR_HIP;
}

// f(Tag<T>) / f(Tag<T>, Tag<TG>) with the storage types of the activations (16-bit) and of the gradient
template <class T>
struct Tag { using type = T; };
template <class F>
static void with_dtype(int dtype, F&& f) {
  if (dtype == DH_DTYPE_F16) f(Tag<f16>{});
  else f(Tag<bf16>{});
}
template <class F>
static void with_dtypes(int dtype, int grad_dtype, F&& f) {
  with_dtype(dtype, [&](auto t) {
    if (grad_dtype == DH_DTYPE_F16) f(t, Tag<f16>{});
    else if (grad_dtype == DH_DTYPE_BF16) f(t, Tag<bf16>{});
    else f(t, Tag<float>{});
  });
}

extern "C" int dh_energy_plan_bytes(int grid, int n_pairs, size_t* bytes) {
  DH_REQUIRE(grid >= 1 && n_pairs >= 0 && bytes, "bad arguments");
  Arena a(nullptr, (size_t)-1);
  EnergyPlan p;
  carve_plan(a, grid, n_pairs, p);
  *bytes = a.off + 256;
  return DH_OK;
}

extern "C" int dh_energy_plan_objects_bytes(int grid, int n_pairs, size_t* bytes) {
  DH_REQUIRE(grid >= 1 && n_pairs >= 0 && bytes, "bad arguments");
  Arena a(nullptr, (size_t)-1);
  EnergyPlanObj p;
  carve_plan_obj(a, grid, n_pairs, p);
  *bytes = a.off + 256;
  return DH_OK;
}

// h: the object header of a weighted plan (then pair_obj and n_objects are read), null for a plain one
static int build_plan(const char* who, const int32_t* pairs, const uint8_t* pair_obj, int n_pairs, const int32_t* bg_trans,
                      int n_bg_trans, int grid, const ObjHeader* h, int n_objects, void* plan, size_t plan_bytes, hipStream_t st) {
  const int G2 = grid * grid;
  const size_t dedupe_lds = (size_t)(G2 + 256) * sizeof(int);
  Arena a(plan, plan_bytes);
  EnergyPlanObj po;
  if (!(h ? carve_plan_obj(a, grid, n_pairs, po) : carve_plan(a, grid, n_pairs, po.base))) return refuse(who, "plan buffer too small");
  const EnergyPlan& p = po.base;
  DH_CHECK_HIP(hipMemsetAsync(p.cnt, 0, (G2 + 1) * sizeof(int), st));
  DH_CHECK_HIP(hipMemsetAsync(p.bgflag, 0, G2, st));
  if (h) hipLaunchKernelGGL(k_store_obj_header, dim3(1), dim3(64), 0, st, *h, po.objp);
  if (n_pairs > 0) hipLaunchKernelGGL(k_hist, dim3(cdiv(n_pairs, 256)), dim3(256), 0, st, pairs, n_pairs, p.cnt, p.w1, p.w2);
  hipLaunchKernelGGL(k_scan_cells, dim3(1), dim3(1024), 0, st, p.cnt, G2, p.off, p.cursor);
  if (n_pairs <= 0) {
    DH_CHECK_HIP(hipMemsetAsync(p.cnt, 0, (G2 + 1) * sizeof(int), st));
  } else if (h) {
    hipLaunchKernelGGL(k_fill_obj, dim3(cdiv(n_pairs, 256)), dim3(256), 0, st, pairs, pair_obj, n_pairs, p.cursor, po.raw);
    hipLaunchKernelGGL(k_dedupe_sources_obj, dim3(G2), dim3(256), dedupe_lds, st, p.off, po.raw, p.src, p.mult,
                       po.objp + OBJ_HEADER, p.cnt, G2, n_objects);
  } else {
    hipLaunchKernelGGL(k_fill, dim3(cdiv(n_pairs, 256)), dim3(256), 0, st, pairs, n_pairs, p.cursor, p.src);
    hipLaunchKernelGGL(k_dedupe_sources, dim3(G2), dim3(256), dedupe_lds, st, p.off, p.src, p.mult, p.cnt, G2);
  }
  if (n_bg_trans > 0) hipLaunchKernelGGL(k_flag_cells, dim3(cdiv(n_bg_trans, 256)), dim3(256), 0, st, bg_trans, n_bg_trans, p.bgflag);
  return launch_status(who);
}

extern "C" int dh_energy_plan_build(const int32_t* pairs, int n_pairs, const int32_t* bg_trans, int n_bg_trans, int grid,
                                    void* plan, size_t plan_bytes, void* stream) {
  DH_REQUIRE(plan && grid >= 1 && n_pairs >= 0 && n_bg_trans >= 0, "bad arguments");
  DH_REQUIRE((size_t)(grid * grid + 256) * sizeof(int) <= 64 * 1024, "grid too large for the dedupe histogram");
  DH_REQUIRE((n_pairs == 0 || pairs) && (n_bg_trans == 0 || bg_trans), "null list");
  return build_plan(__func__, pairs, nullptr, n_pairs, bg_trans, n_bg_trans, grid, nullptr, 0, plan, plan_bytes, (hipStream_t)stream);
}

extern "C" int dh_energy_plan_build_objects(const int32_t* pairs, const uint8_t* pair_obj, int n_pairs, const int32_t* bg_trans,
                                            int n_bg_trans, int grid, int n_objects, const float* weights, const int32_t* counts,
                                            void* plan, size_t plan_bytes, void* stream) {
  DH_REQUIRE(plan && grid >= 1 && n_pairs >= 0 && n_bg_trans >= 0, "bad arguments");
  DH_REQUIRE((size_t)(grid * grid + 256) * sizeof(int) <= 64 * 1024, "grid too large for the dedupe histogram");
  DH_REQUIRE((n_pairs == 0 || (pairs && pair_obj)) && (n_bg_trans == 0 || bg_trans), "null list");
  DH_REQUIRE(n_objects >= 1 && n_objects <= ENERGY_MAX_OBJECTS, "1..8 objects");
  DH_REQUIRE(weights && counts, "null weights or counts");
  double sum = 0.0;
  long long total = 0;
  for (int m = 0; m < n_objects; ++m) {
    DH_REQUIRE(std::isfinite(weights[m]) && weights[m] >= 0.f, "an object weight is negative or not finite");
    DH_REQUIRE(counts[m] >= 0, "negative object count");
    total += counts[m];
    if (counts[m] > 0) sum += (double)weights[m];
  }
  DH_REQUIRE(total == (long long)n_pairs, "the object counts do not add up to n_pairs");
  DH_REQUIRE(n_pairs == 0 || sum > 0.0, "no positive weight among the objects that have pairs");
  ObjHeader h;
  for (int m = 0; m < ENERGY_MAX_OBJECTS; ++m) {
    const bool live = m < n_objects && counts[m] > 0;
    const double om = live ? (double)weights[m] / sum : 0.0;
    h.omega[m] = (float)om;
    h.n[m] = live ? counts[m] : 0;
    h.lossw[m] = live ? om / (double)counts[m] : 0.0;
  }
  return build_plan(__func__, pairs, pair_obj, n_pairs, bg_trans, n_bg_trans, grid, &h, n_objects, plan, plan_bytes, (hipStream_t)stream);
}

extern "C" int dh_energy_planned_workspace_bytes(int C, int grid, size_t* bytes) {
  DH_REQUIRE(C >= 1 && grid >= 1 && bytes, "bad arguments");
  Arena a(nullptr, (size_t)-1);
  PlannedWs w;
  carve_planned(a, C, grid, w);
  *bytes = a.off + 256;
  return DH_OK;
}

extern "C" int dh_energy_planned_batch_workspace_bytes(int C, int grid, int n_items, size_t* bytes) {
  DH_REQUIRE(C >= 1 && grid >= 1 && bytes, "bad arguments");
  DH_REQUIRE(n_items >= 1 && n_items <= ENERGY_MAX_ITEMS, "the batched energy takes 1..16 items");
  Arena a(nullptr, (size_t)-1);
  PlannedWs w;
  for (int e = 0; e < n_items; ++e) carve_planned(a, C, grid, w);
  *bytes = a.off + 256;
  return DH_OK;
}

extern "C" int dh_energy_planned_objects_batch_workspace_bytes(int C, int grid, int n_items, size_t* bytes) {
  return dh_energy_planned_batch_workspace_bytes(C, grid, n_items, bytes);
}

// workgroups of a gradient launch over one item: 256 / (C / 8) cells each
static int grad_blocks(int C, int grid) { return cdiv(grid * grid, 256 / (C / 8)); }

// Checks one item, carves its plan (by its kind; small_plan: the refusal of a buffer that is too small for that kind) and its
// slice of the workspace, and fills its row and its object-block pointer (null: unweighted).  No launch happens here.
static int fill_item(const char* who, const dh_energy_item& in, bool weighted, const char* small_plan, int C, int grid, int nblocks,
                     Arena& aw, EnergyItem& it, const uint8_t*& objp) {
  if (!(in.cur && in.orig && in.grad && in.plan)) return refuse(who, "null pointer in an item");
  if (in.n_pairs < 0) return refuse(who, "bad sizes");
  Arena ap(const_cast<void*>(in.plan), in.plan_bytes);
  EnergyPlanObj po;
  po.objp = nullptr;
  if (!(weighted ? carve_plan_obj(ap, grid, in.n_pairs, po) : carve_plan(ap, grid, in.n_pairs, po.base))) return refuse(who, small_plan);
  const EnergyPlan& p = po.base;
  PlannedWs w;
  if (!carve_planned(aw, C, grid, w)) return refuse(who, "workspace too small");
  const bool bg = in.n_bg_orig > 0 && in.n_bg_trans > 0;
  if (bg && !(in.bg_orig && in.bg_trans)) return refuse(who, "null bg list");
  objp = po.objp;
  it.orig = in.orig; it.cur = in.cur;
  it.off = p.off; it.ucnt = p.cnt; it.src = p.src; it.mult = p.mult; it.bgflag = p.bgflag;
  it.list1 = in.bg_orig; it.list2 = in.bg_trans;
  it.partq = w.partq; it.grad = in.grad; it.loss_part = w.fg_part; it.bg_loss = w.bg_part; it.loss_out = in.loss_out;
  it.n1 = in.n_bg_orig; it.n2 = in.n_bg_trans;
  // weighted: the loss partials carry omega_m / N_m, and the kernel forms fg_w * omega_m / (C N_m) itself from the plain fg_w
  if (weighted) it.fg_norm = in.n_pairs > 0 ? 1.f / (float)C : 0.f;
  else it.fg_norm = in.n_pairs > 0 ? 1.f / ((float)C * (float)in.n_pairs) : 0.f;
  it.coef_fg = weighted ? in.fg_w : in.fg_w * it.fg_norm;
  it.bg_norm = bg ? 1.f / (float)C : 0.f;
  it.coef_bg = bg ? in.bg_w * it.bg_norm / (float)in.n_bg_trans : 0.f;
  it.use_bg = bg ? 1 : 0;
  it.scale = in.grad_scale;
  it.n_fg_part = in.n_pairs > 0 ? nblocks : 0;
  it.fg_w = in.fg_w; it.bg_w = in.bg_w;
  return DH_OK;
}

// ---- one evaluation: the single kernels, their scalar arguments read from the item's row ------------------------------------
// the donor of an item: bits only below the object limit of a plan, and only with a donor pointer
static int check_donor(const char* who, const void* donor, uint32_t donor_objects) {
  if (donor_objects >> ENERGY_MAX_OBJECTS) return refuse(who, "a donor bit at or above the object count of a plan (8 at the most)");
  if (donor_objects && !donor) return refuse(who, "donor objects without donor activations");
  return DH_OK;
}

// donor_objects != 0: the weighted kernel that picks the source rows of the flagged objects from donor (weighted plans only)
static int run_planned_single(const char* who, bool weighted, const dh_energy_item& in, int dtype, int C, int grid, int grad_dtype,
                              void* workspace, size_t workspace_bytes, hipStream_t st, const void* donor = nullptr,
                              uint32_t donor_objects = 0) {
  if (!(in.cur && in.orig && in.grad && in.plan && workspace)) return refuse(who, "null pointer");
  if (const int rc = check_donor(who, donor, donor_objects)) return rc;
  if (!(dtype == DH_DTYPE_F16 || dtype == DH_DTYPE_BF16)) return refuse(who, "the planned path takes 16-bit activations");
  if (!(grad_dtype >= 0 && grad_dtype <= 2)) return refuse(who, "bad dtype");
  if (!(C >= 8 && C % 8 == 0 && C <= 2048 && grid >= 1 && in.n_pairs >= 0)) return refuse(who, "bad sizes");
  const int G2 = grid * grid, nblocks = grad_blocks(C, grid);
  Arena aw(workspace, workspace_bytes);
  EnergyItem it;
  const uint8_t* objp;
  if (const int rc = fill_item(who, in, weighted, "plan buffer too small", C, grid, nblocks, aw, it, objp)) return rc;
  if (it.use_bg)
    with_dtype(dtype, [&](auto t) {
      using T = typename decltype(t)::type;
      hipLaunchKernelGGL((k_colsum_q<T>), dim3(cdiv(C, 64), 4, 2), dim3(8 * CQ_SL), 0, st, (const T*)it.orig, it.list1, it.n1,
                         (const T*)it.cur, it.list2, it.n2, C, it.partq);
    });
  with_dtypes(dtype, grad_dtype, [&](auto t, auto tg) {
    using T = typename decltype(t)::type;
    using TG = typename decltype(tg)::type;
    if (weighted && donor_objects)
      hipLaunchKernelGGL((k_energy_grad_donor<T, TG>), dim3(nblocks), dim3(256), 0, st, (const T*)it.orig, (const T*)donor,
                         (unsigned)donor_objects, (const T*)it.cur, it.off, it.ucnt, it.src, it.mult, objp, it.bgflag, it.partq, it.n1,
                         it.n2, C, G2, it.coef_fg, it.coef_bg, it.use_bg, it.scale, (TG*)it.grad, it.loss_part, it.bg_loss);
    else if (weighted)
      hipLaunchKernelGGL((k_energy_grad_obj<T, TG>), dim3(nblocks), dim3(256), 0, st, (const T*)it.orig, (const T*)it.cur, it.off,
                         it.ucnt, it.src, it.mult, objp, it.bgflag, it.partq, it.n1, it.n2, C, G2, it.coef_fg, it.coef_bg, it.use_bg,
                         it.scale, (TG*)it.grad, it.loss_part, it.bg_loss);
    else
      hipLaunchKernelGGL((k_energy_grad<T, TG>), dim3(nblocks), dim3(256), 0, st, (const T*)it.orig, (const T*)it.cur, it.off,
                         it.ucnt, it.src, it.mult, it.bgflag, it.partq, it.n1, it.n2, C, G2, it.coef_fg, it.coef_bg, it.use_bg,
                         it.scale, (TG*)it.grad, it.loss_part, it.bg_loss);
  });
  if (it.loss_out)
    hipLaunchKernelGGL(k_final_loss, dim3(1), dim3(256), 0, st, it.loss_part, it.n_fg_part, it.fg_norm, it.bg_loss, it.use_bg,
                       it.bg_norm, it.fg_w, it.bg_w, it.loss_out);
  return launch_status(who);
}

extern "C" int dh_energy_fwd_bwd_planned(const void* cur, const void* orig, int dtype, int C, int grid, const void* plan,
                                         size_t plan_bytes, int n_pairs, const int32_t* bg_orig, int n_bg_orig,
                                         const int32_t* bg_trans, int n_bg_trans, float fg_w, float bg_w, float grad_scale,
                                         float* loss_out, void* grad, int grad_dtype, void* workspace,
                                         size_t workspace_bytes, void* stream) {
  const dh_energy_item in = {cur, orig, plan, plan_bytes, bg_orig, bg_trans, loss_out, grad, n_pairs, n_bg_orig, n_bg_trans,
                             fg_w, bg_w, grad_scale};      // (the field order of dh_energy_item)
  return run_planned_single(__func__, false, in, dtype, C, grid, grad_dtype, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int dh_energy_fwd_bwd_planned_objects(const void* cur, const void* orig, int dtype, int C, int grid, const void* plan,
                                                 size_t plan_bytes, int n_pairs, const int32_t* bg_orig, int n_bg_orig,
                                                 const int32_t* bg_trans, int n_bg_trans, float fg_w, float bg_w,
                                                 float grad_scale, float* loss_out, void* grad, int grad_dtype, void* workspace,
                                                 size_t workspace_bytes, void* stream) {
  const dh_energy_item in = {cur, orig, plan, plan_bytes, bg_orig, bg_trans, loss_out, grad, n_pairs, n_bg_orig, n_bg_trans,
                             fg_w, bg_w, grad_scale};      // (the field order of dh_energy_item)
  return run_planned_single(__func__, true, in, dtype, C, grid, grad_dtype, workspace, workspace_bytes, (hipStream_t)stream);
}

// donor_objects = 0 launches what dh_energy_fwd_bwd_planned_objects launches
extern "C" int dh_energy_fwd_bwd_planned_donor(const void* cur, const void* orig, int dtype, int C, int grid, const void* plan,
                                               size_t plan_bytes, int n_pairs, const int32_t* bg_orig, int n_bg_orig,
                                               const int32_t* bg_trans, int n_bg_trans, float fg_w, float bg_w, float grad_scale,
                                               float* loss_out, void* grad, int grad_dtype, void* workspace,
                                               size_t workspace_bytes, void* stream, const void* donor, uint32_t donor_objects) {
  const dh_energy_item in = {cur, orig, plan, plan_bytes, bg_orig, bg_trans, loss_out, grad, n_pairs, n_bg_orig, n_bg_trans,
                             fg_w, bg_w, grad_scale};      // (the field order of dh_energy_item)
  return run_planned_single(__func__, true, in, dtype, C, grid, grad_dtype, workspace, workspace_bytes, (hipStream_t)stream, donor,
                            donor_objects);
}

// ---- K items: one launch pair (plus the loss launch), whichever of the three gradient kernels the entry names ----------------
// k_energy_grad_batch, k_energy_grad_obj_batch, k_energy_grad_mixed_batch, k_energy_grad_donor_batch
enum class BatchKernel { PLAIN, OBJECTS, MIXED, DONOR };

// weighted: one byte per item, non-zero where its plan buffer is a weighted plan (all 0 / all 1 for the two pure entries)
static int run_planned_batch(const char* who, BatchKernel kernel, const dh_energy_item* items, const uint8_t* weighted, int n_items,
                             int dtype, int C, int grid, int grad_dtype, void* workspace, size_t workspace_bytes, hipStream_t st,
                             const EnergyDonorTab* donors = nullptr) {
  if (!(items && weighted && workspace)) return refuse(who, "null pointer");
  if (!(n_items >= 1 && n_items <= ENERGY_MAX_ITEMS))
    return refuse(who, "the batched energy takes 1..16 items (larger batches are not split)");
  if (!(dtype == DH_DTYPE_F16 || dtype == DH_DTYPE_BF16)) return refuse(who, "the planned path takes 16-bit activations");
  if (!(grad_dtype >= 0 && grad_dtype <= 2)) return refuse(who, "bad dtype");
  if (!(C >= 8 && C % 8 == 0 && C <= 2048 && grid >= 1)) return refuse(who, "bad sizes");
  const int G2 = grid * grid, nblocks = grad_blocks(C, grid);
  Arena aw(workspace, workspace_bytes);
  EnergyBatch tab;
  EnergyObjPtrs ot;
  bool any_bg = false, any_loss = false;
  for (int e = 0; e < n_items; ++e) {
    // only the mixed entry says which kind of plan was too small
    const char* small_plan = kernel == BatchKernel::MIXED && weighted[e] ? "plan buffer too small for a weighted plan" : "plan buffer too small";
    if (const int rc = fill_item(who, items[e], weighted[e] != 0, small_plan, C, grid, nblocks, aw, tab.it[e], ot.p[e])) return rc;
    any_bg = any_bg || tab.it[e].use_bg;
    any_loss = any_loss || tab.it[e].loss_out != nullptr;
  }
  for (int e = n_items; e < ENERGY_MAX_ITEMS; ++e) { tab.it[e] = tab.it[0]; ot.p[e] = ot.p[0]; }      // (never indexed: defined kernel arguments)
  if (any_bg)
    with_dtype(dtype, [&](auto t) {
      using T = typename decltype(t)::type;
      hipLaunchKernelGGL((k_colsum_q_batch<T>), dim3(cdiv(C, 64), 4, 2 * n_items), dim3(8 * CQ_SL), 0, st, tab, C);
    });
  with_dtypes(dtype, grad_dtype, [&](auto t, auto tg) {
    using T = typename decltype(t)::type;
    using TG = typename decltype(tg)::type;
    const dim3 blocks(nblocks, n_items);
    if (kernel == BatchKernel::PLAIN) hipLaunchKernelGGL((k_energy_grad_batch<T, TG>), blocks, dim3(256), 0, st, tab, C, G2);
    else if (kernel == BatchKernel::OBJECTS) hipLaunchKernelGGL((k_energy_grad_obj_batch<T, TG>), blocks, dim3(256), 0, st, tab, ot, C, G2);
    else if (kernel == BatchKernel::DONOR) hipLaunchKernelGGL((k_energy_grad_donor_batch<T, TG>), blocks, dim3(256), 0, st, tab, ot, *donors, C, G2);
    else hipLaunchKernelGGL((k_energy_grad_mixed_batch<T, TG>), blocks, dim3(256), 0, st, tab, ot, C, G2);
  });
  if (any_loss) hipLaunchKernelGGL(k_final_loss_batch, dim3(n_items), dim3(256), 0, st, tab);
  return launch_status(who);
}

extern "C" int dh_energy_fwd_bwd_planned_batch(const dh_energy_item* items, int n_items, int dtype, int C, int grid,
                                               int grad_dtype, void* workspace, size_t workspace_bytes, void* stream) {
  static const uint8_t none[ENERGY_MAX_ITEMS] = {};
  return run_planned_batch(__func__, BatchKernel::PLAIN, items, none, n_items, dtype, C, grid, grad_dtype, workspace, workspace_bytes,
                           (hipStream_t)stream);
}

extern "C" int dh_energy_fwd_bwd_planned_objects_batch(const dh_energy_item* items, int n_items, int dtype, int C, int grid,
                                                       int grad_dtype, void* workspace, size_t workspace_bytes, void* stream) {
  static_assert(ENERGY_MAX_ITEMS == 16, "one flag per item");
  static const uint8_t all[ENERGY_MAX_ITEMS] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1};
  return run_planned_batch(__func__, BatchKernel::OBJECTS, items, all, n_items, dtype, C, grid, grad_dtype, workspace, workspace_bytes,
                           (hipStream_t)stream);
}

extern "C" int dh_energy_fwd_bwd_planned_mixed_batch(const dh_energy_item* items, const uint8_t* weighted, int n_items, int dtype,
                                                     int C, int grid, int grad_dtype, void* workspace, size_t workspace_bytes,
                                                     void* stream) {
  return run_planned_batch(__func__, BatchKernel::MIXED, items, weighted, n_items, dtype, C, grid, grad_dtype, workspace, workspace_bytes,
                           (hipStream_t)stream);
}

// K weighted items, each with its donor (null with no bit set: that item computes what the objects batch computes for it)
extern "C" int dh_energy_fwd_bwd_planned_donor_batch(const dh_energy_donor_item* items, int n_items, int dtype, int C, int grid,
                                                     int grad_dtype, void* workspace, size_t workspace_bytes, void* stream) {
  static const uint8_t all[ENERGY_MAX_ITEMS] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1};
  if (!items) return refuse(__func__, "null pointer");
  if (!(n_items >= 1 && n_items <= ENERGY_MAX_ITEMS))
    return refuse(__func__, "the batched energy takes 1..16 items (larger batches are not split)");
  dh_energy_item plain[ENERGY_MAX_ITEMS];
  EnergyDonorTab dt;
  for (int e = 0; e < ENERGY_MAX_ITEMS; ++e) {
    const dh_energy_donor_item& in = items[e < n_items ? e : 0];      // (rows past n_items are never indexed: defined arguments)
    if (const int rc = check_donor(__func__, in.donor, in.donor_objects)) return rc;
    plain[e] = in.item;
    dt.donor[e] = in.donor_objects ? in.donor : in.item.orig;
    dt.bits[e] = in.donor_objects;
  }
  return run_planned_batch(__func__, BatchKernel::DONOR, plain, all, n_items, dtype, C, grid, grad_dtype, workspace, workspace_bytes,
                           (hipStream_t)stream, &dt);
}
