// Small f32 kernels of the denoising loops: CFG combine + DDIM step, latent update,
// Adam step on the null-text embedding, MSE and its gradient.
#include "common.h"

namespace dh {

__global__ void k_ddim_cfg(float* out, const float* x, const float* eu, const float* ec, float scale, float sa_t,
                           float s1a_t, float sa_p, float s1a_p, int n) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float e = ec[i];
  if (eu) { float u = eu[i]; e = u + scale * (e - u); }
  float x0 = (x[i] - s1a_t * e) / sa_t;
  out[i] = sa_p * x0 + s1a_p * e;
}

__global__ void k_latent_update(float* out, const float* x, const float* g, float k, int n) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = x[i] - k * g[i];
}

__global__ void k_latent_update_s(float* out, const float* x, const float* g, int gc, int c, float k, int n) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int p = i / c, ch = i - p * c;
  out[i] = x[i] - k * g[(size_t)p * gc + ch];
}

__global__ void k_pack_sample(float* dst, const float* lat, int lb, int cl, const float* dep, int db, int cd, int pixels, int n) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int ct = cl + cd;
  const int ch = i % ct, r = i / ct, p = r % pixels, b = r / pixels;
  dst[i] = ch < cl ? lat[((size_t)(b % lb) * pixels + p) * cl + ch]
                   : dep[((size_t)(b % db) * pixels + p) * cd + (ch - cl)];
}

__global__ void k_adam(float* p, const float* g, float* m, float* v, float lr, float b1, float b2, float eps,
                       float bc1, float bc2_sqrt, int n) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float gi = g[i];
  float mi = m[i] + (1.f - b1) * (gi - m[i]);          // lerp form used by torch
  float vi = b2 * v[i] + (1.f - b2) * gi * gi;
  m[i] = mi;
  v[i] = vi;
  float denom = sqrtf(vi) / bc2_sqrt + eps;
  p[i] = p[i] - (lr / bc1) * (mi / denom);
}

// one workgroup: the latent has 16 K - 300 K elements, and a single-block reduction needs no partials buffer
// (nothing process-global, legal inside stream capture, deterministic summation order)
__global__ void __launch_bounds__(1024) k_mse(const float* a, const float* b, int n, float* out, float* d_a) {
  __shared__ double sm[16];
  double l = 0.0;
  const float k = 2.f / (float)n;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    float d = a[i] - b[i];
    l += (double)d * (double)d;
    if (d_a) d_a[i] = k * d;
  }
  l = block_sum(l, sm);
  if (threadIdx.x == 0) out[0] = (float)(l / (double)n);
}

// mse(a, b) and the cotangent of a 16-bit backward pass seeded by it: d_eps = (2 (a - b) / n) * k * S, S = the power of
// two that brings max |d_eps| into (amp / 2, amp].  The engine's backward is linear in its cotangent, so S cancels exactly
// in g / S; what it buys is range: fp16 products of a 1e-6-sized cotangent fall into the subnormals (measured at the full
// SD-2-depth size, tools/probe_text_grad.py: d_text error 2.4e-3 for max |d_eps| >= 1, 1.9e-2 at 2^-4, 9e-2 at 2^-8).
__global__ void __launch_bounds__(1024) k_mse_cotangent(const float* a, const float* b, int n, float k, float amp, float* loss_out,
                                                        float* d_eps, float* scale_out) {
  __shared__ double sm[16];
  __shared__ float smax[16];
  double l = 0.0;
  float mx = 0.f;
  const float k2 = 2.f / (float)n;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const float d = a[i] - b[i];
    l += (double)d * (double)d;
    mx = fmaxf(mx, fabsf(k2 * d));
  }
  l = block_sum(l, sm);
  mx = wave_max(mx);
  if ((threadIdx.x & 63) == 0) smax[threadIdx.x >> 6] = mx;
  __syncthreads();
  mx = 0.f;
  for (int w = 0; w < (int)((blockDim.x + 63) >> 6); ++w) mx = fmaxf(mx, smax[w]);
  mx *= fabsf(k);
  float S = 1.f;
  if (amp > 0.f && mx > 0.f && mx < INFINITY) {
    int e = 0;
    (void)frexpf(amp / mx, &e);           // amp / mx = f * 2^e with f in [0.5, 1): 2^(e-1) <= amp / mx
    e = e - 1;
    e = e > 100 ? 100 : (e < -100 ? -100 : e);
    S = ldexpf(1.f, e);
  }
  const float kS = k * S;
  for (int i = threadIdx.x; i < n; i += blockDim.x) d_eps[i] = (k2 * (a[i] - b[i])) * kS;
  if (threadIdx.x == 0) { loss_out[0] = (float)(l / (double)n); scale_out[0] = S; }
}

__global__ void k_adam_scaled(float* p, const float* g, float* m, float* v, float lr, float b1, float b2, float eps,
                              float bc1, float bc2_sqrt, const float* g_scale, int n) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float gi = g[i] / g_scale[0];
  // an overflowed 16-bit backward pass (inf / NaN in the text gradient) must not poison the embedding for every later
  // timestep: such an element keeps its parameter and moments for this step
  if (!isfinite(gi)) return;
  float mi = m[i] + (1.f - b1) * (gi - m[i]);
  float vi = b2 * v[i] + (1.f - b2) * gi * gi;
  m[i] = mi;
  v[i] = vi;
  float denom = sqrtf(vi) / bc2_sqrt + eps;
  p[i] = p[i] - (lr / bc1) * (mi / denom);
}

// k_mse_cotangent for `batch` images of n elements each, one workgroup per image (blockIdx.x = image), with the early stop of
// the null-text inner loop: an image inactive on entry gets d_eps = 0 and S = 1 (its loss is still written); updated[b] =
// active[b] on entry, active[b] &= !((double)loss < threshold).  Workgroup b alone reads and writes active[b] / updated[b].
__global__ void __launch_bounds__(1024) k_mse_cotangent_batch(const float* a_all, const float* b_all, int n, float k, float amp,
                                                              double threshold, int* active, int* updated, float* loss_out,
                                                              float* d_eps_all, float* scale_out) {
  __shared__ double sm[16];
  __shared__ float smax[16];
  const int img = blockIdx.x;
  const size_t off = (size_t)img * n;
  const float* a = a_all + off;
  const float* b = b_all + off;
  float* d_eps = d_eps_all + off;
  const int on = active[img];           // read by every thread before the barriers below; written once after them
  double l = 0.0;
  float mx = 0.f;
  const float k2 = 2.f / (float)n;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const float d = a[i] - b[i];
    l += (double)d * (double)d;
    mx = fmaxf(mx, fabsf(k2 * d));
  }
  l = block_sum(l, sm);
  mx = wave_max(mx);
  if ((threadIdx.x & 63) == 0) smax[threadIdx.x >> 6] = mx;
  __syncthreads();
  mx = 0.f;
  for (int w = 0; w < (int)((blockDim.x + 63) >> 6); ++w) mx = fmaxf(mx, smax[w]);
  mx *= fabsf(k);
  float S = 1.f;
  if (on && amp > 0.f && mx > 0.f && mx < INFINITY) {
    int e = 0;
    (void)frexpf(amp / mx, &e);
    e = e - 1;
    e = e > 100 ? 100 : (e < -100 ? -100 : e);
    S = ldexpf(1.f, e);
  }
  const float kS = k * S;
  if (on) {
    for (int i = threadIdx.x; i < n; i += blockDim.x) d_eps[i] = (k2 * (a[i] - b[i])) * kS;
  } else {
    for (int i = threadIdx.x; i < n; i += blockDim.x) d_eps[i] = 0.f;
  }
  if (threadIdx.x == 0) {
    const float loss = (float)(l / (double)n);
    loss_out[img] = loss;
    scale_out[img] = S;
    updated[img] = on;
    active[img] = (on && !((double)loss < threshold)) ? 1 : 0;
  }
}

// k_adam_scaled on image blockIdx.y of `batch` (n elements each), skipped as a whole where updated[image] == 0
__global__ void k_adam_scaled_batch(float* p, const float* g, float* m, float* v, float lr, float b1, float b2, float eps,
                                    float bc1, float bc2_sqrt, const float* g_scale, const int* updated, int n) {
  const int img = blockIdx.y;
  if (!updated[img]) return;
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const size_t j = (size_t)img * n + i;
  float gi = g[j] / g_scale[img];
  if (!isfinite(gi)) return;
  float mi = m[j] + (1.f - b1) * (gi - m[j]);
  float vi = b2 * v[j] + (1.f - b2) * gi * gi;
  m[j] = mi;
  v[j] = vi;
  float denom = sqrtf(vi) / bc2_sqrt + eps;
  p[j] = p[j] - (lr / bc1) * (mi / denom);
}


// ---- guarded forms of the guided loop's update and DDIM step ('auto' guidance scale) -------------------------------
// Status of an edit: int[4] = {kinds seen (bit 0: backward overflow, update held; bit 1: non-finite latent after the DDIM
// step), number of held updates, code of the first failure ((t_idx + 1) << 16 | (iteration & 0xff) << 8 | kind; 0 = none),
// 0}.  Written with ordinary global stores / atomics, only on failure.
constexpr int GU_THREADS = 1024, GU_PER = 48;      // one workgroup holds an edit of up to 48 K elements in registers (96^2 x 4 = 36 K)
__device__ __forceinline__ bool nonfinite_bits(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }
__device__ __forceinline__ int status_code(int t_idx, int iteration, int kind) {
  return ((t_idx + 1) << 16) | ((iteration & 0xff) << 8) | kind;
}

// one workgroup per edit (blockIdx.x): out = x - (lr / S_e) * g if the edit's gradient slice is finite, else out = x and the
// edit's status records the held update.  g: [pixels][gc] per edit, the first c channels of every pixel; S_e =
// scale[e * tab_stride + tab_index] (a power of two).  Every element of g is read once, into registers.
__global__ void __launch_bounds__(GU_THREADS) k_latent_update_guarded(float* out, const float* x, const float* g, int gc, int c,
                                                                      int n, float lr, const float* scale, int tab_stride,
                                                                      int tab_index, int* status, float* gmax, int t_idx,
                                                                      int iteration) {
  __shared__ int sbad[GU_THREADS / 64];
  __shared__ float smax[GU_THREADS / 64];
  const int e = blockIdx.x, tid = threadIdx.x;
  const float* ge = g + (size_t)e * (n / c) * gc;
  const float* xe = x + (size_t)e * n;
  float* oe = out + (size_t)e * n;
  float v[GU_PER];
  int bad = 0;
  float mx = 0.f;
#pragma unroll
  for (int j = 0; j < GU_PER; ++j) {
    const int i = tid + j * GU_THREADS;
    v[j] = 0.f;
    if (i < n) {
      const int p = i / c, ch = i - p * c;
      v[j] = ge[(size_t)p * gc + ch];
      bad |= nonfinite_bits(v[j]) ? 1 : 0;
      mx = fmaxf(mx, fabsf(v[j]));
    }
  }
  bad = wave_max(bad);
  mx = wave_max(mx);
  if ((tid & 63) == 0) { sbad[tid >> 6] = bad; smax[tid >> 6] = mx; }
  __syncthreads();
  bad = 0;
  mx = 0.f;
  for (int w = 0; w < GU_THREADS / 64; ++w) { bad |= sbad[w]; mx = fmaxf(mx, smax[w]); }
  const float S = scale[(size_t)e * tab_stride + tab_index];
  if (!bad) {
    int ex = 0;
    (void)frexpf(S, &ex);
    const float k = ldexpf(lr, 1 - ex);          // lr / S, exact for a power of two S
#pragma unroll
    for (int j = 0; j < GU_PER; ++j) {
      const int i = tid + j * GU_THREADS;
      if (i < n) oe[i] = xe[i] - k * v[j];
    }
  } else {
#pragma unroll
    for (int j = 0; j < GU_PER; ++j) {
      const int i = tid + j * GU_THREADS;
      if (i < n) oe[i] = xe[i];
    }
  }
  if (tid == 0) {
    if (gmax) gmax[e] = bad ? NAN : mx / S;
    if (bad) {
      int* st = status + 4 * e;
      st[0] |= 1;
      st[1] += 1;
      if (st[2] == 0) st[2] = status_code(t_idx, iteration, 1);
    }
  }
}

// k_ddim_cfg, and bit 1 of the status of edit i / n_edit where an output element is not finite: a wave ballot, then one lane
// per (wave, failing edit) does the global atomics -- nothing is written while the outputs are finite
__global__ void k_ddim_cfg_flagged(float* out, const float* x, const float* eu, const float* ec, float scale, float sa_t,
                                   float s1a_t, float sa_p, float s1a_p, int n, int n_edit, int* status, int t_idx,
                                   int iteration) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool valid = i < n;
  bool bad = false;
  if (valid) {
    float e = ec[i];
    if (eu) { float u = eu[i]; e = u + scale * (e - u); }
    float x0 = (x[i] - s1a_t * e) / sa_t;
    const float o = sa_p * x0 + s1a_p * e;
    out[i] = o;
    bad = nonfinite_bits(o);
  }
  const int edit = valid ? i / n_edit : 0;
  const int lane = threadIdx.x & 63;
  unsigned long long m = __ballot(bad);
  while (m) {
    const int l = __ffsll((long long)m) - 1;
    const int el = __shfl(edit, l, 64);
    if (lane == l) {
      atomicOr(&status[4 * el], 2);
      atomicCAS(&status[4 * el + 2], 0, status_code(t_idx, iteration, 2));
    }
    m &= ~__ballot(bad && edit == el);
  }
}

// ---- background lock: the DDIM step blended with the reconstruction outside the edit's region -----------------------
// The item table travels by value in the kernel arguments (the idiom of energy.hip); the item is a block index, so its row
// is read through scalar loads.
constexpr int LOCK_MAX_ITEMS = 16;
struct LockTable {
  dh_lock_item it[LOCK_MAX_ITEMS];
};

// grid (blocks of an edit's elements, edits).  o = k_ddim_cfg's value; out = o where keep == 0 or the edit is not locked,
// the reconstruction r where keep == 1, o + keep (r - o) in between.  status (may be NULL): bit 1 of the edit's word where
// o -- the step BEFORE the blend -- is not finite, as k_ddim_cfg_flagged sets it.
__global__ void k_ddim_cfg_locked(float* out, const float* x, const float* eu, const float* ec, float scale, float sa_t,
                                  float s1a_t, float sa_p, float s1a_p, int n_edit, int channels, const LockTable tab,
                                  int* status, int t_idx, int iteration) {
  const int edit = blockIdx.y;
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  const float* keep = tab.it[edit].keep;
  const float* ref = tab.it[edit].ref;
  bool bad = false;
  if (j < n_edit) {
    const size_t i = (size_t)edit * n_edit + j;
    float e = ec[i];
    if (eu) { float u = eu[i]; e = u + scale * (e - u); }
    float x0 = (x[i] - s1a_t * e) / sa_t;
    const float o = sa_p * x0 + s1a_p * e;
    bad = nonfinite_bits(o);
    float v = o;
    if (keep) {
      const float k = keep[j / channels];
      if (k >= 1.f) v = ref[j];
      else if (k > 0.f) v = o + k * (ref[j] - o);
    }
    out[i] = v;
  }
  if (status && __ballot(bad) && (threadIdx.x & 63) == 0) {
    atomicOr(&status[4 * edit], 2);
    atomicCAS(&status[4 * edit + 2], 0, status_code(t_idx, iteration, 2));
  }
}

}  // namespace dh
using namespace dh;

extern "C" int dh_ddim_cfg_step_locked(float* x_out, const float* x, const float* eps_u, const float* eps_c, float scale,
                                       float alpha_t, float alpha_prev, int n, int n_edit, int channels,
                                       const dh_lock_item* items, int n_items, int* status, int t_idx, int iteration,
                                       void* stream) {
  DH_REQUIRE(x_out && x && eps_c && items && n > 0 && n_edit > 0 && n % n_edit == 0 && channels > 0 && n_edit % channels == 0 &&
             t_idx >= 0 && t_idx < 32767 && iteration >= 0, "bad arguments");
  DH_REQUIRE(n_items >= 1 && n_items <= LOCK_MAX_ITEMS, "1 to 16 items (one per edit; never split)");
  DH_REQUIRE(n_items == n / n_edit, "one item per edit of the batch");
  LockTable tab;
  for (int e = 0; e < LOCK_MAX_ITEMS; ++e) tab.it[e] = dh_lock_item{nullptr, nullptr};
  for (int e = 0; e < n_items; ++e) {
    DH_REQUIRE(!items[e].keep || items[e].ref, "a locked item needs its reconstruction latent");
    tab.it[e] = items[e];
  }
  float sa_t = sqrtf(alpha_t), s1a_t = sqrtf(1.f - alpha_t), sa_p = sqrtf(alpha_prev), s1a_p = sqrtf(1.f - alpha_prev);
  hipLaunchKernelGGL(k_ddim_cfg_locked, dim3(cdiv(n_edit, 256), n_items), dim3(256), 0, (hipStream_t)stream, x_out, x, eps_u,
                     eps_c, scale, sa_t, s1a_t, sa_p, s1a_p, n_edit, channels, tab, status, t_idx, iteration);
  DH_LAUNCH_CHECK();
  return DH_OK;
}

extern "C" int dh_ddim_cfg_step(float* x_out, const float* x, const float* eps_u, const float* eps_c, float scale,
                                float alpha_t, float alpha_prev, int n, void* stream) {
  DH_REQUIRE(x_out && x && eps_c && n > 0, "bad arguments");
  // torch evaluates a**0.5 on float32 0-d tensors: float32 sqrt of the float32 alpha
  float sa_t = sqrtf(alpha_t), s1a_t = sqrtf(1.f - alpha_t), sa_p = sqrtf(alpha_prev), s1a_p = sqrtf(1.f - alpha_prev);
  hipLaunchKernelGGL(k_ddim_cfg, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, x_out, x, eps_u, eps_c, scale,
                     sa_t, s1a_t, sa_p, s1a_p, n);
  DH_LAUNCH_CHECK();
  return DH_OK;
}

extern "C" int dh_latent_update(float* x_out, const float* x, const float* g, float lr, float grad_scale, int n,
                                void* stream) {
  DH_REQUIRE(x_out && x && g && n > 0 && grad_scale != 0.f, "bad arguments");
  hipLaunchKernelGGL(k_latent_update, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, x_out, x, g,
                     lr / grad_scale, n);
  DH_LAUNCH_CHECK();
  return DH_OK;
}

extern "C" int dh_adam_step(float* p, const float* g, float* m, float* v, float lr, float beta1, float beta2,
                            float eps, int step, int n, void* stream) {
  DH_REQUIRE(p && g && m && v && n > 0 && step >= 1, "bad arguments");
  float bc1 = 1.f - powf(beta1, (float)step);
  float bc2 = sqrtf(1.f - powf(beta2, (float)step));
  hipLaunchKernelGGL(k_adam, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, lr, beta1, beta2, eps,
                     bc1, bc2, n);
  DH_LAUNCH_CHECK();
  return DH_OK;
}

extern "C" int dh_mse_fwd_bwd(const float* rec, const float* target, int n, float* loss_out, float* d_rec,
                              void* stream) {
  DH_REQUIRE(rec && target && loss_out && n > 0, "bad arguments");
  hipLaunchKernelGGL(k_mse, dim3(1), dim3(1024), 0, (hipStream_t)stream, rec, target, n, loss_out, d_rec);
  DH_LAUNCH_CHECK();
  return DH_OK;
}

extern "C" int dh_mse_cotangent(const float* rec, const float* target, int n, float k, float amp, float* loss_out,
                                float* d_eps, float* scale_out, void* stream) {
  DH_REQUIRE(rec && target && loss_out && d_eps && scale_out && n > 0, "bad arguments");
  hipLaunchKernelGGL(k_mse_cotangent, dim3(1), dim3(1024), 0, (hipStream_t)stream, rec, target, n, k, amp, loss_out, d_eps,
                     scale_out);
  DH_LAUNCH_CHECK();
  return DH_OK;
}

extern "C" int dh_adam_step_scaled(float* p, const float* g, const float* g_scale, float* m, float* v, float lr, float beta1,
                                   float beta2, float eps, int step, int n, void* stream) {
  DH_REQUIRE(p && g && g_scale && m && v && n > 0 && step >= 1, "bad arguments");
  float bc1 = 1.f - powf(beta1, (float)step);
  float bc2 = sqrtf(1.f - powf(beta2, (float)step));
  hipLaunchKernelGGL(k_adam_scaled, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, lr, beta1, beta2,
                     eps, bc1, bc2, g_scale, n);
  DH_LAUNCH_CHECK();
  return DH_OK;
}

extern "C" int dh_mse_cotangent_batch(const float* rec, const float* target, int batch, int n, float k, float amp,
                                      double threshold, int* active, int* updated, float* loss_out, float* d_eps,
                                      float* scale_out, void* stream) {
  DH_REQUIRE(rec && target && active && updated && loss_out && d_eps && scale_out && batch >= 1 && n > 0, "bad arguments");
  hipLaunchKernelGGL(k_mse_cotangent_batch, dim3(batch), dim3(1024), 0, (hipStream_t)stream, rec, target, n, k, amp,
                     threshold, active, updated, loss_out, d_eps, scale_out);
  DH_LAUNCH_CHECK();
  return DH_OK;
}

extern "C" int dh_adam_step_scaled_batch(float* p, const float* g, const float* g_scale, const int* updated, float* m, float* v,
                                         float lr, float beta1, float beta2, float eps, int step, int batch, int n,
                                         void* stream) {
  DH_REQUIRE(p && g && g_scale && updated && m && v && batch >= 1 && batch <= 65535 && n > 0 && step >= 1, "bad arguments");
  float bc1 = 1.f - powf(beta1, (float)step);
  float bc2 = sqrtf(1.f - powf(beta2, (float)step));
  hipLaunchKernelGGL(k_adam_scaled_batch, dim3(cdiv(n, 256), batch), dim3(256), 0, (hipStream_t)stream, p, g, m, v, lr, beta1,
                     beta2, eps, bc1, bc2, g_scale, updated, n);
  DH_LAUNCH_CHECK();
  return DH_OK;
}

extern "C" int dh_latent_update_strided(float* x_out, const float* x, const float* g, int g_channels, int channels, float lr,
                                        float grad_scale, int pixels, void* stream) {
  DH_REQUIRE(x_out && x && g && pixels > 0 && channels > 0 && g_channels >= channels && grad_scale != 0.f, "bad arguments");
  const int n = pixels * channels;
  hipLaunchKernelGGL(k_latent_update_s, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, x_out, x, g, g_channels, channels,
                     lr / grad_scale, n);
  DH_LAUNCH_CHECK();
  return DH_OK;
}

extern "C" int dh_pack_sample(float* dst, const float* latent, int latent_batch, int latent_channels, const float* depth,
                              int depth_batch, int depth_channels, int batch, int pixels, void* stream) {
  DH_REQUIRE(dst && latent && batch >= 1 && pixels > 0 && latent_channels > 0, "bad arguments");
  DH_REQUIRE(latent_batch >= 1 && batch % latent_batch == 0 && (!depth || (depth_batch >= 1 && batch % depth_batch == 0)),
             "latent / depth batches must divide the batch (item b reads item b mod its batch)");
  const int cd = depth ? depth_channels : 0;
  DH_REQUIRE(!depth || cd > 0, "depth without channels");
  const int n = batch * pixels * (latent_channels + cd);
  hipLaunchKernelGGL(k_pack_sample, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, dst, latent, latent_batch,
                     latent_channels, depth, depth_batch, cd, pixels, n);
  DH_LAUNCH_CHECK();
  return DH_OK;
}

extern "C" int dh_latent_update_guarded(float* x_out, const float* x, const float* g, int g_channels, int channels, float lr,
                                        int pixels, int edits, const float* scale_table, int table_stride, int table_index,
                                        int* status, float* gmax, int t_idx, int iteration, void* stream) {
  DH_REQUIRE(x_out && x && g && scale_table && status && pixels > 0 && channels > 0 && g_channels >= channels && edits >= 1 &&
             table_stride >= 1 && table_index >= 0 && table_index < table_stride && t_idx >= 0 && t_idx < 32767 && iteration >= 0,
             "bad arguments");
  DH_REQUIRE((long long)pixels * channels <= (long long)GU_THREADS * GU_PER, "latent too large for one workgroup per edit");
  hipLaunchKernelGGL(k_latent_update_guarded, dim3(edits), dim3(GU_THREADS), 0, (hipStream_t)stream, x_out, x, g, g_channels,
                     channels, pixels * channels, lr, scale_table, table_stride, table_index, status, gmax, t_idx, iteration);
  DH_LAUNCH_CHECK();
  return DH_OK;
}

extern "C" int dh_ddim_cfg_step_flagged(float* x_out, const float* x, const float* eps_u, const float* eps_c, float scale,
                                        float alpha_t, float alpha_prev, int n, int n_edit, int* status, int t_idx, int iteration,
                                        void* stream) {
  DH_REQUIRE(x_out && x && eps_c && status && n > 0 && n_edit > 0 && n % n_edit == 0 && t_idx >= 0 && t_idx < 32767 &&
             iteration >= 0, "bad arguments");
  float sa_t = sqrtf(alpha_t), s1a_t = sqrtf(1.f - alpha_t), sa_p = sqrtf(alpha_prev), s1a_p = sqrtf(1.f - alpha_prev);
  hipLaunchKernelGGL(k_ddim_cfg_flagged, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, x_out, x, eps_u, eps_c, scale,
                     sa_t, s1a_t, sa_p, s1a_p, n, n_edit, status, t_idx, iteration);
  DH_LAUNCH_CHECK();
  return DH_OK;
}
