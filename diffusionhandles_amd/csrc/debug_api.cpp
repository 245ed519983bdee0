// Test hooks: C-ABI wrappers around the individual kernel launchers so that the GPU parity
// tests can check each kernel against a torch fp32 reference in isolation.  Not used by the
// product path.
#include <stdlib.h>

#include <cstring>
#include <vector>

#include "unet_kernels.h"
using namespace dh;

// ---- arena hooks (host only; tests/test_arena_hooks.py, tests/test_workspace_guards_gpu.py) ------------------------------------
// Plain globals like the CG cap and the footprint tier: set by a test, read by every Arena (common.h), reset by the test.
namespace dh {
size_t g_arena_gap = 0;
bool g_arena_log = false;
static std::vector<int64_t> g_arena_takes;        // (base address, offset, bytes) per take
void arena_log_take(const void* base, size_t off, size_t bytes) {
  g_arena_takes.push_back((int64_t)(intptr_t)base);
  g_arena_takes.push_back((int64_t)off);
  g_arena_takes.push_back((int64_t)bytes);
}
}  // namespace dh
// every take of every arena, in the size queries and in the entries alike, skips `bytes` behind its sub-buffer: a band no
// kernel may touch.  0 (the default) is the product's layout byte for byte.
extern "C" int dh_dbg_arena_gap(int bytes) {
  DH_REQUIRE(bytes >= 0 && bytes <= 65536 && bytes % 256 == 0, "the gap is 0 or a multiple of 256 up to 65536");
  dh::g_arena_gap = (size_t)bytes;
  return DH_OK;
}
// enable != 0: clear the log and record every take from now on (a query's null-based arena logs base 0); 0: stop recording
extern "C" int dh_dbg_arena_log(int enable) {
  if (enable) dh::g_arena_takes.clear();
  dh::g_arena_log = enable != 0;
  return DH_OK;
}
// out [cap][3] = (base address, offset, bytes) of the first min(cap, *n) takes, *n = the takes recorded
extern "C" int dh_dbg_arena_log_read(int64_t* out, int cap, int* n) {
  DH_REQUIRE(n && cap >= 0 && (cap == 0 || out), "bad arguments");
  const size_t have = dh::g_arena_takes.size() / 3;
  for (size_t i = 0; i < have && i < (size_t)cap; ++i)
    for (int j = 0; j < 3; ++j) out[3 * i + j] = dh::g_arena_takes[3 * i + j];
  *n = (int)have;
  return DH_OK;
}

// the members of a dh_reproject_args as this library reads them, in declaration order: integers by value, floats, doubles and
// pointers by bit pattern (the ctypes twin in _lib.py is compared against it).  *n = the members there are
extern "C" int dh_dbg_reproject_args(const dh_reproject_args* a, int64_t* out, int cap, int* n) {
  DH_REQUIRE(a && n && cap >= 0 && (cap == 0 || out), "bad arguments");
  std::vector<int64_t> v;
  auto bits = [&](auto x) {
    int64_t b = 0;
    static_assert(sizeof x <= sizeof b, "a member wider than 64 bits");
    memcpy(&b, &x, sizeof x);
    v.push_back(b);
  };
  for (int64_t x : {(int64_t)a->struct_bytes, (int64_t)a->res, (int64_t)a->n_fg, (int64_t)a->n_objects, (int64_t)a->n_edits,
                    (int64_t)a->n_instances, (int64_t)a->n_bones, (int64_t)a->corr_capacity, (int64_t)a->footprints,
                    (int64_t)a->n_donor_objects, (int64_t)a->infill_border, (int64_t)a->view_surfaces})
    v.push_back(x);
  bits(a->max_ratio), bits(a->surface_max_ratio), bits(a->inv_fx), bits(a->inv_fy), bits(a->fx), bits(a->fy);
  bits(a->depth), bits(a->bg_depth), bits(a->fg_pix), bits(a->grid_x), bits(a->grid_y), bits(a->bounds), bits(a->donor_depth);
  bits(a->bg_valid), bits(a->bone_w);
  bits(a->obj_start), bits(a->inst_obj), bits(a->xforms_host), bits(a->views), bits(a->has_view);
  bits(a->zmap), bits(a->raw_mask), bits(a->clean_mask), bits(a->disparity), bits(a->vis), bits(a->target_xy), bits(a->corr);
  bits(a->corr_inst), bits(a->counts), bits(a->bg_corr), bits(a->bg_counts);
  bits(a->workspace), bits(a->workspace_bytes), bits(a->stream);
  for (size_t i = 0; i < v.size() && i < (size_t)cap; ++i) out[i] = v[i];
  *n = (int)v.size();
  return DH_OK;
}

static void* g_dbg_tiled = nullptr;     // the tiled copy of the last weight matrix dh_dbg_gemm was given

// timing runs (tools/bench_gemm_warmth.py): one streaming read over the tiled weights, i.e. what a prefetch would leave in the caches
__global__ void k_dbg_touch(const uint4* p, size_t n16, unsigned* sink) {
  unsigned acc = 0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (size_t)gridDim.x * blockDim.x) { const uint4 v = p[i]; acc ^= v.x ^ v.y ^ v.z ^ v.w; }
  if (acc == 0x9e3779b9u && sink) sink[0] = acc;
}
extern "C" int dh_dbg_touch_tiled(size_t bytes, void* stream) {
  DH_REQUIRE(g_dbg_tiled != nullptr, "no tiled weights yet (call dh_dbg_gemm first)");
  hipLaunchKernelGGL(k_dbg_touch, dim3(512), dim3(256), 0, (hipStream_t)stream, (const uint4*)g_dbg_tiled, bytes / 16, (unsigned*)nullptr);
  DH_LAUNCH_CHECK();
  return DH_OK;
}

// dh_dbg_gemm with the convolution's top / left zero padding as an argument (GemmArgs::pad; 0 with stride 2 = the VAE encoder's
// down-sampler, which pads bottom / right only)
extern "C" int dh_dbg_gemm_pad(int dtype, const void* A, long lda, const void* W, int M, int N, int K, int mode, int Hin,
                               int Win, int Cin, int Hout, int Wout, int stride, int up, int pad, const float* bias,
                               const float* rowvec, int rowvec_ld, int rows_per_batch, const void* R, long ldr, void* C,
                               long ldc, int act_silu, float* partial, size_t partial_elems, void* stream) {
  DH_REQUIRE(A && W && C && K % 64 == 0 && N % 64 == 0, "bad arguments (N, K must be multiples of 64)");
  // the hook takes plain [N][K] weights and tiles them into a scratch buffer first
  void*& tiled = g_dbg_tiled;
  static size_t tiled_cap = 0;
  static const void* tiled_from = nullptr;
  const size_t need = (size_t)N * K * 2;
  if (need > tiled_cap) {
    if (tiled) (void)hipFree(tiled);
    DH_CHECK_HIP(hipMalloc(&tiled, need));
    tiled_cap = need;
    tiled_from = nullptr;
  }
  static const bool pretiled = getenv("DH_DBG_PRETILED") != nullptr;   // timing runs: tile a weight matrix once, not per call
  if (!pretiled || tiled_from != W) launch_tile_weights(dtype, W, tiled, N, K, (hipStream_t)stream, mode != 0 ? Cin : 0);
  tiled_from = W;
  GemmArgs g;
  g.A = A; g.lda = lda; g.W = tiled; g.M = M; g.N = N; g.K = K; g.mode = mode; g.Hin = Hin; g.Win = Win; g.Cin = Cin;
  g.Hout = Hout; g.Wout = Wout; g.stride = stride; g.up = up; g.pad = pad; g.bias = bias; g.rowvec = rowvec; g.rowvec_ld = rowvec_ld;
  g.rows_per_batch = rows_per_batch; g.R = R; g.ldr = ldr; g.C = C; g.ldc = ldc; g.act_silu = act_silu;
  g.partial = partial; g.partial_elems = partial_elems;
  launch_gemm(dtype, g, (hipStream_t)stream);
  DH_LAUNCH_CHECK();
  return DH_OK;
}
// ... with the usual padding of 1 (the hook's original signature, kept for its existing callers)
extern "C" int dh_dbg_gemm(int dtype, const void* A, long lda, const void* W, int M, int N, int K, int mode, int Hin,
                           int Win, int Cin, int Hout, int Wout, int stride, int up, const float* bias,
                           const float* rowvec, int rowvec_ld, int rows_per_batch, const void* R, long ldr, void* C,
                           long ldc, int act_silu, float* partial, size_t partial_elems, void* stream) {
  return dh_dbg_gemm_pad(dtype, A, lda, W, M, N, K, mode, Hin, Win, Cin, Hout, Wout, stride, up, 1, bias, rowvec, rowvec_ld,
                         rows_per_batch, R, ldr, C, ldc, act_silu, partial, partial_elems, stream);
}
// GEMM (dense or 3x3 convolution) followed by the GroupNorm(+SiLU) of its output, the way the engine's forward runs the pair: the
// GroupNorm's slice statistics come from the GEMM launch when it can leave them (split-K reduce, or -- round 6 -- the epilogue of an
// unsplit k_gemm_dma launch: gemm.hip gn_epi) and from the statistics kernel otherwise.  *have_out = what the GEMM reported
// (0 = statistics kernel, 1 = reduce, > 1 = slices left by the epilogue); stats [B * G][2] = (mean, rstd).  R (row pitch ldr) is
// the residual added before rounding, or NULL; it may be C itself (in place, as the engine's resnet shortcut adds run).
extern "C" int dh_dbg_gemm_groupnorm_geo(int dtype, const void* A, long lda, const void* W, int M, int N, int K, int mode, int Hin, int Win,
                                         int Cin, int Hout, int Wout, int stride, int up, const float* bias, const float* rowvec, int rowvec_ld,
                                         int rows_per_batch, const void* R, long ldr, void* C, float* partial, size_t partial_elems, int HW, int G,
                                         const float* gamma, const float* beta, float eps, int silu, void* Y, float* stats, float* scratch,
                                         int* have_out, void* stream) {
  DH_REQUIRE(A && W && C && Y && stats && scratch && gamma && beta && K % 64 == 0 && N % 64 == 0 && HW > 0 && M % HW == 0, "bad arguments");
  static void* tiled = nullptr;        // (this hook's own tiled copy: dh_dbg_gemm keeps the capacity of ITS buffer)
  static size_t cap = 0;
  const size_t need = (size_t)N * K * 2;
  if (need > cap) {
    if (tiled) (void)hipFree(tiled);
    DH_CHECK_HIP(hipMalloc(&tiled, need));
    cap = need;
  }
  launch_tile_weights(dtype, W, tiled, N, K, (hipStream_t)stream, mode != 0 ? Cin : 0);
  GemmArgs g;
  g.A = A; g.lda = lda; g.W = tiled; g.M = M; g.N = N; g.K = K; g.mode = mode; g.Hin = Hin; g.Win = Win; g.Cin = Cin;
  g.Hout = Hout; g.Wout = Wout; g.stride = stride; g.up = up; g.bias = bias; g.rowvec = rowvec; g.rowvec_ld = rowvec_ld;
  g.rows_per_batch = rows_per_batch; g.R = R; g.ldr = ldr; g.C = C; g.ldc = N;
  g.partial = partial; g.partial_elems = partial_elems;
  int have = 0;
  g.gn_part = scratch; g.gn_HW = HW; g.gn_G = G; g.gn_done = &have;
  launch_gemm(dtype, g, (hipStream_t)stream);
  launch_groupnorm_fwd(dtype, C, gamma, beta, Y, stats, scratch, M / HW, HW, N, G, eps, silu, (hipStream_t)stream, have);
  if (have_out) *have_out = have;
  DH_LAUNCH_CHECK();
  return DH_OK;
}
// ... a stride-1 convolution without up-sampling or a dense GEMM, no per-image vector (the hook's signature before
// dh_dbg_gemm_groupnorm_geo took the whole geometry, kept for its existing callers)
extern "C" int dh_dbg_gemm_groupnorm_res(int dtype, const void* A, long lda, const void* W, int M, int N, int K, int mode, int Hin, int Win,
                                     int Cin, const float* bias, const void* R, long ldr, void* C, float* partial, size_t partial_elems, int HW, int G,
                                     const float* gamma, const float* beta, float eps, int silu, void* Y, float* stats, float* scratch,
                                     int* have_out, void* stream) {
  return dh_dbg_gemm_groupnorm_geo(dtype, A, lda, W, M, N, K, mode, Hin, Win, Cin, Hin, Win, 1, 0, bias, nullptr, 0, 1, R, ldr, C, partial,
                                   partial_elems, HW, G, gamma, beta, eps, silu, Y, stats, scratch, have_out, stream);
}
// ... without a residual (the hook's original signature, kept for its existing callers)
extern "C" int dh_dbg_gemm_groupnorm(int dtype, const void* A, long lda, const void* W, int M, int N, int K, int mode, int Hin, int Win,
                                     int Cin, const float* bias, void* C, float* partial, size_t partial_elems, int HW, int G,
                                     const float* gamma, const float* beta, float eps, int silu, void* Y, float* stats, float* scratch,
                                     int* have_out, void* stream) {
  return dh_dbg_gemm_groupnorm_res(dtype, A, lda, W, M, N, K, mode, Hin, Win, Cin, bias, nullptr, N, C, partial, partial_elems, HW, G,
                                   gamma, beta, eps, silu, Y, stats, scratch, have_out, stream);
}
// ... and the backward twin: C = A W^T is dy of GroupNorm(x) (+ SiLU) with saved (mean, rstd) in `stats`; the GEMM (its split-K
// reduce, or its own epilogue: *have_out > 1 = that many slices per group) leaves the backward slice statistics in `scratch` and
// the GroupNorm backward writes dx.  (engine: every input-gradient GEMM in front of a GroupNorm backward; R = C, pitch ldr, when the
// gradient already holds a contribution it accumulates onto -- NULL otherwise)
extern "C" int dh_dbg_gemm_groupnorm_bwd_geo(int dtype, const void* A, long lda, const void* W, int M, int N, int K, int mode, int Hin,
                                             int Win, int Cin, int Hout, int Wout, int stride, int up, const void* R, long ldr, void* C,
                                             float* partial, size_t partial_elems, int HW, int G, const void* x, const float* gamma,
                                             const float* beta, const float* stats, int silu, void* dx, float* scratch, int* have_out,
                                             void* stream) {
  DH_REQUIRE(A && W && C && x && dx && stats && scratch && gamma && beta && K % 64 == 0 && N % 64 == 0 && HW > 0 && M % HW == 0, "bad arguments");
  static void* tiled = nullptr;
  static size_t cap = 0;
  const size_t need = (size_t)N * K * 2;
  if (need > cap) {
    if (tiled) (void)hipFree(tiled);
    DH_CHECK_HIP(hipMalloc(&tiled, need));
    cap = need;
  }
  launch_tile_weights(dtype, W, tiled, N, K, (hipStream_t)stream, mode != 0 ? Cin : 0);
  GemmArgs g;
  g.A = A; g.lda = lda; g.W = tiled; g.M = M; g.N = N; g.K = K; g.mode = mode; g.Hin = Hin; g.Win = Win; g.Cin = Cin;
  g.Hout = Hout; g.Wout = Wout; g.stride = stride; g.up = up; g.R = R; g.ldr = ldr; g.C = C; g.ldc = N;
  g.partial = partial; g.partial_elems = partial_elems;
  int have = 0;
  g.gnb_x = x; g.gnb_ldx = N; g.gnb_gamma = gamma; g.gnb_beta = beta; g.gnb_stats = stats; g.gnb_silu = silu;
  g.gn_part = scratch; g.gn_HW = HW; g.gn_G = G; g.gn_done = &have;
  launch_gemm(dtype, g, (hipStream_t)stream);
  launch_groupnorm_bwd(dtype, x, C, gamma, beta, stats, dx, scratch, M / HW, HW, N, G, silu, 0, (hipStream_t)stream, have, GnBwdSplit());
  if (have_out) *have_out = have;
  DH_LAUNCH_CHECK();
  return DH_OK;
}
// ... a stride-1 convolution without up-sampling or a dense GEMM (the hook's signature before dh_dbg_gemm_groupnorm_bwd_geo took the
// whole geometry, kept for its existing callers)
extern "C" int dh_dbg_gemm_groupnorm_bwd_res(int dtype, const void* A, long lda, const void* W, int M, int N, int K, int mode, int Hin,
                                         int Win, int Cin, const void* R, long ldr, void* C, float* partial, size_t partial_elems, int HW, int G, const void* x,
                                         const float* gamma, const float* beta, const float* stats, int silu, void* dx,
                                         float* scratch, int* have_out, void* stream) {
  return dh_dbg_gemm_groupnorm_bwd_geo(dtype, A, lda, W, M, N, K, mode, Hin, Win, Cin, Hin, Win, 1, 0, R, ldr, C, partial, partial_elems, HW, G, x,
                                       gamma, beta, stats, silu, dx, scratch, have_out, stream);
}
// ... without a residual (the hook's original signature, kept for its existing callers)
extern "C" int dh_dbg_gemm_groupnorm_bwd(int dtype, const void* A, long lda, const void* W, int M, int N, int K, int mode, int Hin,
                                         int Win, int Cin, void* C, float* partial, size_t partial_elems, int HW, int G, const void* x,
                                         const float* gamma, const float* beta, const float* stats, int silu, void* dx,
                                         float* scratch, int* have_out, void* stream) {
  return dh_dbg_gemm_groupnorm_bwd_res(dtype, A, lda, W, M, N, K, mode, Hin, Win, Cin, nullptr, N, C, partial, partial_elems, HW, G, x,
                                       gamma, beta, stats, silu, dx, scratch, have_out, stream);
}
// channel concatenation a | b followed by the GroupNorm(+SiLU) of the result, the way the engine's forward runs OP_CONCAT in front
// of a GroupNorm: k_concat_gn writes out [B * HW][Ca + Cb] and the slice statistics, the apply kernel merges them.
// stats [B * G][2] = (mean, rstd); scratch holds the slices.
extern "C" int dh_dbg_concat_groupnorm(int dtype, const void* a, int Ca, const void* b, int Cb, void* out, int B, int HW, int G,
                                       const float* gamma, const float* beta, float eps, int silu, void* Y, float* stats,
                                       float* scratch, void* stream) {
  DH_REQUIRE(a && b && out && Y && stats && scratch && gamma && beta && B > 0 && HW > 0 && G > 0, "bad arguments");
  DH_REQUIRE(Ca % 8 == 0 && Cb % 8 == 0 && (Ca + Cb) % G == 0 && (GN_GB * ((Ca + Cb) / G)) % 8 == 0 && GN_GB * ((Ca + Cb) / G) <= 2048,
             "shape the fused concatenation does not take");
  launch_concat_gn(dtype, a, Ca, b, Cb, out, scratch, B, HW, G, (hipStream_t)stream);
  launch_groupnorm_fwd(dtype, out, gamma, beta, Y, stats, scratch, B, HW, Ca + Cb, G, eps, silu, (hipStream_t)stream, 1);
  DH_LAUNCH_CHECK();
  return DH_OK;
}
// the LayerNorm-folded form of the dense GEMM (engine: qkv / cross-attention q / GEGLU in-projection at B <= 3): A is the
// LayerNorm INPUT, W already carries gamma, ln_s[n] = sum_k W[n][k], ln_t[n] = sum_k beta[k] W0[n][k] (+ bias);
// out = rstd (A W^T - mean ln_s) + ln_t, and (mean, rstd) per row land in ln_stats
extern "C" int dh_dbg_gemm_lnfold(int dtype, const void* A, long lda, const void* W, int M, int N, int K, const float* ln_s,
                                  const float* ln_t, float* ln_stats, float ln_eps, void* C, long ldc, void* stream) {
  DH_REQUIRE(A && W && C && ln_s && ln_t && ln_stats && K % 64 == 0 && N % 64 == 0, "bad arguments (N, K must be multiples of 64)");
  static void* tiled = nullptr;
  static size_t tiled_cap = 0;
  const size_t need = (size_t)N * K * 2;
  if (need > tiled_cap) {
    if (tiled) (void)hipFree(tiled);
    DH_CHECK_HIP(hipMalloc(&tiled, need));
    tiled_cap = need;
  }
  launch_tile_weights(dtype, W, tiled, N, K, (hipStream_t)stream);
  GemmArgs g;
  g.A = A; g.lda = lda; g.W = tiled; g.M = M; g.N = N; g.K = K; g.mode = A_DENSE; g.C = C; g.ldc = ldc;
  g.ln_s = ln_s; g.ln_t = ln_t; g.ln_stats = ln_stats; g.ln_eps = ln_eps;
  launch_gemm(dtype, g, (hipStream_t)stream);
  DH_LAUNCH_CHECK();
  return DH_OK;
}
// q projection + cross-attention the way the engine's forward runs attn2 (head dim 64, H = N / 64 heads, B images of M / B queries):
// q = A W^T (+ bias), or the LayerNorm-folded form when ln_s is given (see dh_dbg_gemm_lnfold); o [M][N] = softmax(q K^T / 8) V per
// head over the Nk keys of the row's image (k / v: [B * Nk][ldk], head h at column 64 h), lse [B][H][M / B].  The GEMM's dispatch
// decides whether its epilogue carries the attention (*carried = 1: one launch, and q is written only when save != 0) or the
// attention kernel runs behind it (*carried = 0).
extern "C" int dh_dbg_gemm_xattn(int dtype, const void* A, long lda, const void* W, int M, int N, int K, const float* bias,
                                 const float* ln_s, const float* ln_t, float* ln_stats, float ln_eps, void* q, const void* k,
                                 const void* v, long ldk, void* o, float* lse, int B, int Nk, int save, int* carried, void* stream) {
  DH_REQUIRE(A && W && q && k && v && o && lse && K % 64 == 0 && N % 64 == 0 && B > 0 && M % B == 0 && Nk > 0, "bad arguments");
  DH_REQUIRE(!ln_s || (ln_t && ln_stats), "the folded LayerNorm needs ln_s, ln_t and ln_stats");
  static void* tiled = nullptr;
  static size_t tiled_cap = 0;
  const size_t need = (size_t)N * K * 2;
  if (need > tiled_cap) {
    if (tiled) (void)hipFree(tiled);
    DH_CHECK_HIP(hipMalloc(&tiled, need));
    tiled_cap = need;
  }
  launch_tile_weights(dtype, W, tiled, N, K, (hipStream_t)stream);
  GemmArgs g;
  g.A = A; g.lda = lda; g.W = tiled; g.M = M; g.N = N; g.K = K; g.mode = A_DENSE; g.bias = bias; g.C = q; g.ldc = N;
  if (ln_s) { g.ln_s = ln_s; g.ln_t = ln_t; g.ln_stats = ln_stats; g.ln_eps = ln_eps; }
  int have = 0;
  g.xa_k = k; g.xa_v = v; g.xa_ldk = ldk; g.xa_o = o; g.xa_ldo = N; g.xa_lse = lse; g.xa_H = N / 64; g.xa_Nq = M / B; g.xa_Nk = Nk;
  g.xa_save = save; g.xa_done = &have;
  launch_gemm(dtype, g, (hipStream_t)stream);
  if (!have) launch_attention_fwd(dtype, q, N, k, v, ldk, o, N, lse, B, N / 64, M / B, Nk, (hipStream_t)stream);
  if (carried) *carried = have;
  DH_LAUNCH_CHECK();
  return DH_OK;
}
// ... and the backward to q the way the engine runs it when no text gradient is wanted: dO = A W^T [M][N] (the input-gradient GEMM
// of attn2.to_out.0) and dq of the cross-attention with saved q, o [M][N], lse and k / v as above.  *carried = 1: the GEMM's
// epilogue wrote dq and d_o is untouched; *carried = 0: d_o holds dO and the dQ kernel ran behind the GEMM.
extern "C" int dh_dbg_gemm_xattn_dq(int dtype, const void* A, long lda, const void* W, int M, int N, int K, void* d_o, const void* q,
                                    const void* k, const void* v, long ldk, const void* o, const float* lse, void* dq, int B, int Nk,
                                    int* carried, void* stream) {
  DH_REQUIRE(A && W && d_o && q && k && v && o && lse && dq && K % 64 == 0 && N % 64 == 0 && B > 0 && M % B == 0 && Nk > 0, "bad arguments");
  static void* tiled = nullptr;
  static size_t tiled_cap = 0;
  const size_t need = (size_t)N * K * 2;
  if (need > tiled_cap) {
    if (tiled) (void)hipFree(tiled);
    DH_CHECK_HIP(hipMalloc(&tiled, need));
    tiled_cap = need;
  }
  launch_tile_weights(dtype, W, tiled, N, K, (hipStream_t)stream);
  GemmArgs g;
  g.A = A; g.lda = lda; g.W = tiled; g.M = M; g.N = N; g.K = K; g.mode = A_DENSE; g.C = d_o; g.ldc = N;
  int have = 0;
  g.xa_k = k; g.xa_v = v; g.xa_ldk = ldk; g.xa_o = const_cast<void*>(o); g.xa_ldo = N; g.xa_lse = const_cast<float*>(lse);
  g.xa_H = N / 64; g.xa_Nq = M / B; g.xa_Nk = Nk; g.xa_q = q; g.xa_ldq = N; g.xa_dq = dq; g.xa_lddq = N; g.xa_done = &have;
  launch_gemm(dtype, g, (hipStream_t)stream);
  if (!have) launch_attention_bwd_dq(dtype, q, N, k, v, ldk, o, N, d_o, N, lse, nullptr, dq, N, B, N / 64, M / B, Nk, (hipStream_t)stream);
  if (carried) *carried = have;
  DH_LAUNCH_CHECK();
  return DH_OK;
}
// the GEGLU epilogues of the dense GEMM (engine: ff.net.0.proj forward, ff.net.2 input-gradient).  bwd = 0: W [N = 2F][K] and bias
// in the PAIRED row order (unet_kernels.h glu_col), C (may be NULL) receives the pre-activations [M][2F] (paired), y [M][F] =
// value * gelu(gate).  bwd = 1: the GEMM's tile A W^T [M][N = F] is dy of a GEGLU with saved pre-activations x [M][2F] (paired);
// dx [M][2F] (paired) receives d_value | d_gate.
extern "C" int dh_dbg_gemm_glu(int dtype, int bwd, const void* A, long lda, const void* W, int M, int N, int K, const float* bias,
                               void* C, void* y, const void* x, void* dx, void* stream) {
  DH_REQUIRE(A && W && K % 64 == 0 && N % 128 == 0, "bad arguments (K % 64, N % 128)");
  DH_REQUIRE(bwd ? (x && dx) : (y != nullptr), "missing output");
  static void* tiled = nullptr;
  static size_t tiled_cap = 0;
  const size_t need = (size_t)N * K * 2;
  if (need > tiled_cap) {
    if (tiled) (void)hipFree(tiled);
    DH_CHECK_HIP(hipMalloc(&tiled, need));
    tiled_cap = need;
  }
  launch_tile_weights(dtype, W, tiled, N, K, (hipStream_t)stream);
  GemmArgs g;
  g.A = A; g.lda = lda; g.W = tiled; g.M = M; g.N = N; g.K = K; g.mode = A_DENSE; g.bias = bias;
  if (bwd) { g.glub_x = x; g.glub_dx = dx; }
  else { g.C = C; g.ldc = N; g.glu_y = y; g.glu_ldy = N / 2; }
  launch_gemm(dtype, g, (hipStream_t)stream);
  DH_LAUNCH_CHECK();
  return DH_OK;
}
// the GEGLU forward epilogue on a LayerNorm-folded GEMM (engine: ff.net.0.proj at B <= 3): A is the LayerNorm input, W [N = 2F][K]
// carries gamma, ln_s / ln_t as dh_dbg_gemm_lnfold takes them (the bias inside ln_t), all three in the PAIRED row order; C (may be
// NULL) receives the pre-activations [M][2F] (paired), y [M][F] = value * gelu(gate), ln_stats [M][2] = (mean, rstd)
extern "C" int dh_dbg_gemm_lnfold_glu(int dtype, const void* A, long lda, const void* W, int M, int N, int K, const float* ln_s,
                                      const float* ln_t, float* ln_stats, float ln_eps, void* C, void* y, void* stream) {
  DH_REQUIRE(A && W && y && ln_s && ln_t && ln_stats && K % 64 == 0 && N % 128 == 0, "bad arguments (K % 64, N % 128)");
  static void* tiled = nullptr;
  static size_t tiled_cap = 0;
  const size_t need = (size_t)N * K * 2;
  if (need > tiled_cap) {
    if (tiled) (void)hipFree(tiled);
    DH_CHECK_HIP(hipMalloc(&tiled, need));
    tiled_cap = need;
  }
  launch_tile_weights(dtype, W, tiled, N, K, (hipStream_t)stream);
  GemmArgs g;
  g.A = A; g.lda = lda; g.W = tiled; g.M = M; g.N = N; g.K = K; g.mode = A_DENSE; g.C = C; g.ldc = N;
  g.ln_s = ln_s; g.ln_t = ln_t; g.ln_stats = ln_stats; g.ln_eps = ln_eps;
  g.glu_y = y; g.glu_ldy = N / 2;
  launch_gemm(dtype, g, (hipStream_t)stream);
  DH_LAUNCH_CHECK();
  return DH_OK;
}
// input-gradient GEMM -> LayerNorm backward the way the engine's backward pass runs the pair: dy = A W^T [M][N] is the gradient of
// LayerNorm(x) (x: row pitch ldx, saved (mean, rstd) in stats [M][2]); dx [M][N] = the LayerNorm's input gradient (+ add when
// given).  *done_out = 1: the split-K reduce of the GEMM applied the backward to the summed rows and dy is untouched; 0: dy
// holds the GEMM's output and the LayerNorm backward ran behind it.
extern "C" int dh_dbg_gemm_layernorm_bwd(int dtype, const void* A, long lda, const void* W, int M, int N, int K, const void* x, long ldx,
                                         const float* gamma, const float* stats, const void* add, void* dy, void* dx, float* partial,
                                         size_t partial_elems, int* done_out, void* stream) {
  DH_REQUIRE(A && W && x && gamma && stats && dy && dx && K % 64 == 0 && N % 64 == 0 && ldx >= N, "bad arguments (N, K must be multiples of 64)");
  DH_REQUIRE(N <= LN_MAX_C, "N must be <= " + std::to_string(LN_MAX_C) + " (LayerNorm row width)");
  static void* tiled = nullptr;
  static size_t tiled_cap = 0;
  const size_t need = (size_t)N * K * 2;
  if (need > tiled_cap) {
    if (tiled) (void)hipFree(tiled);
    DH_CHECK_HIP(hipMalloc(&tiled, need));
    tiled_cap = need;
  }
  launch_tile_weights(dtype, W, tiled, N, K, (hipStream_t)stream);
  GemmArgs g;
  g.A = A; g.lda = lda; g.W = tiled; g.M = M; g.N = N; g.K = K; g.mode = A_DENSE; g.C = dy; g.ldc = N;
  g.partial = partial; g.partial_elems = partial_elems;
  int done = 0;
  g.lnb_x = x; g.lnb_ldx = ldx; g.lnb_gamma = gamma; g.lnb_stats = stats; g.lnb_add = add; g.lnb_dx = dx; g.lnb_done = &done;
  launch_gemm(dtype, g, (hipStream_t)stream);
  if (!done) launch_layernorm_bwd(dtype, x, dy, gamma, stats, add, dx, M, N, (hipStream_t)stream, ldx);
  if (done_out) *done_out = done;
  DH_LAUNCH_CHECK();
  return DH_OK;
}
extern "C" int dh_dbg_gemm_last_tile(int* out);
// the column-split GEGLU backward (engine: the input-gradient GEMM of a transformer's proj_out folded into ff.net.2).  W [N][K]
// plain; the tile A W^T [M][N] holds dy of a GEGLU in columns [0, F) (saved pre-activations x [M][2F], paired; dx [M][2F]
// receives d_value | d_gate) and a plain output in columns [F, N), which goes to C [M][N - F] (row stride ldc; accumulate = 1 adds
// it to what C holds).  tile (if set) receives dh_dbg_gemm_last_tile's nine values of the launch.
extern "C" int dh_dbg_gemm_glub_split(int dtype, const void* A, long lda, const void* W, int M, int N, int K, int F, void* C,
                                      long ldc, int accumulate, const void* x, void* dx, int* tile, void* stream) {
  DH_REQUIRE(A && W && C && x && dx && K % 64 == 0 && N % 64 == 0 && F % 64 == 0 && F > 0 && F < N, "bad arguments (K, N, F % 64; 0 < F < N)");
  static void* tiled = nullptr;
  static size_t tiled_cap = 0;
  const int Np = (int)align_up((size_t)N, 128);     // whole 128-row tiles, zero past N (what the engine's folded weight holds)
  const size_t need = (size_t)Np * K * 2;
  if (need > tiled_cap) {
    if (tiled) (void)hipFree(tiled);
    DH_CHECK_HIP(hipMalloc(&tiled, need));
    tiled_cap = need;
  }
  DH_CHECK_HIP(hipMemsetAsync(tiled, 0, need, (hipStream_t)stream));
  launch_tile_weights(dtype, W, tiled, N, K, (hipStream_t)stream);
  GemmArgs g;
  g.A = A; g.lda = lda; g.W = tiled; g.M = M; g.N = N; g.K = K; g.mode = A_DENSE;
  g.glub_x = x; g.glub_dx = dx; g.glub_f = F;
  g.C = C; g.ldc = ldc;
  if (accumulate) { g.R = C; g.ldr = ldc; }
  launch_gemm(dtype, g, (hipStream_t)stream);
  if (tile) dh_dbg_gemm_last_tile(tile);
  DH_LAUNCH_CHECK();
  return DH_OK;
}
extern "C" int dh_dbg_groupnorm(int dtype, const void* x, const float* gamma, const float* beta, void* y, float* stats,
                                const void* dy, void* dx, float* scratch, int B, int HW, int C, int G, float eps,
                                int silu, int accumulate, void* stream) {
  launch_groupnorm_fwd(dtype, x, gamma, beta, y, stats, scratch, B, HW, C, G, eps, silu, (hipStream_t)stream);
  if (dy && dx)
    launch_groupnorm_bwd(dtype, x, dy, gamma, beta, stats, dx, scratch, B, HW, C, G, silu, accumulate, (hipStream_t)stream);
  DH_LAUNCH_CHECK();
  return DH_OK;
}
// the row widths k_ln_fwd / k_ln_bwd hold (unet_kernels.h LN_MAX_C)
static bool ln_width_ok(int C) { return C >= 8 && C % 8 == 0 && C <= LN_MAX_C; }
static std::string ln_width_text() { return "C must be a multiple of 8 and <= " + std::to_string(LN_MAX_C) + " (LayerNorm row width)"; }
extern "C" int dh_dbg_layernorm(int dtype, const void* x, const float* gamma, const float* beta, void* y, float* stats,
                                const void* dy, const void* add, void* dx, int rows, int C, float eps, void* stream) {
  DH_REQUIRE(ln_width_ok(C), ln_width_text());
  launch_layernorm_fwd(dtype, x, gamma, beta, y, stats, rows, C, eps, (hipStream_t)stream);
  if (dy && dx) launch_layernorm_bwd(dtype, x, dy, gamma, stats, add, dx, rows, C, (hipStream_t)stream);
  DH_LAUNCH_CHECK();
  return DH_OK;
}
// dh_dbg_layernorm with x at row pitch ldx (elements, >= C; y, dy, add and dx stay dense), the way the engine passes a tensor's
// pitch to both launchers.  stats may be NULL for a forward alone; add may be NULL or alias dx.
extern "C" int dh_dbg_layernorm_ld(int dtype, const void* x, long ldx, const float* gamma, const float* beta, void* y, float* stats,
                                   const void* dy, const void* add, void* dx, int rows, int C, float eps, void* stream) {
  DH_REQUIRE(ln_width_ok(C), ln_width_text());
  DH_REQUIRE(x && gamma && beta && y && rows >= 1 && ldx >= C && ldx % 8 == 0, "bad arguments (ldx >= C, ldx % 8 == 0)");
  DH_REQUIRE(!(dy && dx) || stats, "the backward reads the saved statistics: stats must not be NULL");
  launch_layernorm_fwd(dtype, x, gamma, beta, y, stats, rows, C, eps, (hipStream_t)stream, ldx);
  if (dy && dx) launch_layernorm_bwd(dtype, x, dy, gamma, stats, add, dx, rows, C, (hipStream_t)stream, ldx);
  DH_LAUNCH_CHECK();
  return DH_OK;
}
extern "C" int dh_dbg_geglu(int dtype, const void* x, void* y, const void* dy, void* dx, int rows, int F, void* stream) {
  DH_REQUIRE(F >= 16 && F % 16 == 0, "F must be a positive multiple of 16 (paired column layout)");
  launch_geglu_fwd(dtype, x, y, rows, F, (hipStream_t)stream);
  if (dy && dx) launch_geglu_bwd(dtype, x, dy, dx, rows, F, (hipStream_t)stream);
  DH_LAUNCH_CHECK();
  return DH_OK;
}
extern "C" int dh_dbg_attention(int dtype, const void* q, long ldq, const void* k, const void* v, long ldk, void* o,
                                long ldo, float* lse, const void* d_o, float* delta, void* dq, void* dk, void* dv,
                                int B, int H, int Nq, int Nk, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  launch_attention_fwd(dtype, q, ldq, k, v, ldk, o, ldo, lse, B, H, Nq, Nk, st);
  if (d_o) {
    if (dq) launch_attention_bwd_dq(dtype, q, ldq, k, v, ldk, o, ldo, d_o, ldo, lse, delta, dq, ldq, B, H, Nq, Nk, st);
    else launch_attention_delta(dtype, o, ldo, d_o, ldo, delta, B, H, Nq, st);
    if (dk && dv) {
      static float* scratch = nullptr;                 // test hook only: lets the query-chunk path of the few-key case run
      constexpr size_t kScratch = (size_t)16 << 20;
      if (!scratch && hipMalloc((void**)&scratch, kScratch * sizeof(float)) != hipSuccess) scratch = nullptr;
      launch_attention_bwd_dkv(dtype, q, ldq, k, v, ldk, d_o, ldo, lse, delta, dk, dv, ldk, B, H, Nq, Nk, st, scratch,
                               scratch ? kScratch : 0);
    }
  }
  DH_LAUNCH_CHECK();
  return DH_OK;
}
// attention backward of one layer, dQ and dK/dV either one after the other on `stream` (stream2 == NULL: dQ writes delta, dK/dV
// reads it) or SIDE BY SIDE: delta by its own kernel, then dQ on `stream` and dK/dV on `stream2` between a fork and a join event
// (measurement hook: what the two kernels gain from each other's idle CUs at B = 1)
extern "C" int dh_dbg_attention_bwd_pair(int dtype, const void* q, long ldq, const void* k, const void* v, long ldk, const void* o,
                                         long ldo, const float* lse, const void* d_o, float* delta, void* dq, void* dk, void* dv,
                                         int B, int H, int Nq, int Nk, void* stream, void* stream2) {
  hipStream_t st = (hipStream_t)stream, s2 = (hipStream_t)stream2;
  if (!s2) {
    launch_attention_bwd_dq(dtype, q, ldq, k, v, ldk, o, ldo, d_o, ldo, lse, delta, dq, ldq, B, H, Nq, Nk, st);
    launch_attention_bwd_dkv(dtype, q, ldq, k, v, ldk, d_o, ldo, lse, delta, dk, dv, ldk, B, H, Nq, Nk, st, nullptr, 0);
  } else {
    static hipEvent_t fork = nullptr, join = nullptr;
    if (!fork) { DH_CHECK_HIP(hipEventCreateWithFlags(&fork, hipEventDisableTiming)); DH_CHECK_HIP(hipEventCreateWithFlags(&join, hipEventDisableTiming)); }
    launch_attention_delta(dtype, o, ldo, d_o, ldo, delta, B, H, Nq, st);
    DH_CHECK_HIP(hipEventRecord(fork, st));
    DH_CHECK_HIP(hipStreamWaitEvent(s2, fork, 0));
    launch_attention_bwd_dkv(dtype, q, ldq, k, v, ldk, d_o, ldo, lse, delta, dk, dv, ldk, B, H, Nq, Nk, s2, nullptr, 0);
    launch_attention_bwd_dq(dtype, q, ldq, k, v, ldk, o, ldo, d_o, ldo, lse, nullptr, dq, ldq, B, H, Nq, Nk, st);
    DH_CHECK_HIP(hipEventRecord(join, s2));
    DH_CHECK_HIP(hipStreamWaitEvent(st, join, 0));
  }
  DH_LAUNCH_CHECK();
  return DH_OK;
}
extern "C" int dh_dbg_pool2x2(int dtype, const void* src, void* dst, int B, int h, int w, int C, int accumulate, void* stream) {
  launch_pool2x2_sum(dtype, src, dst, B, h, w, C, accumulate, (hipStream_t)stream);
  DH_LAUNCH_CHECK();
  return DH_OK;
}
extern "C" int dh_dbg_lane_ops(const float* in, float* out, unsigned* ex, void* stream) {
  launch_lane_ops_probe(in, out, ex, (hipStream_t)stream);
  DH_LAUNCH_CHECK();
  return DH_OK;
}
// ---- hooks for the kernels that only the engines launch (tests/test_engine_kernels_gpu.py)
// the forward with the causal mask (text tower: key j visible to query i for j <= i); lse may be NULL, as the text engine passes it
extern "C" int dh_dbg_attention_causal(int dtype, const void* q, long ldq, const void* k, const void* v, long ldk, void* o, long ldo,
                                       float* lse, int B, int H, int Nq, int Nk, void* stream) {
  DH_REQUIRE(q && k && v && o, "bad arguments");
  launch_attention_fwd(dtype, q, ldq, k, v, ldk, o, ldo, lse, B, H, Nq, Nk, (hipStream_t)stream, 1);
  DH_LAUNCH_CHECK();
  return DH_OK;
}
// the two tiny-channel convolutions through their launchers: bwd = 0 launch_conv_small_fwd (x_is_f32 picks few-in, else few-out),
// bwd = 1 launch_conv_small_bwd (x = dy, y = dx, w = the gradient convolution's weights, Cin / Cout those of that convolution;
// bias and y_is_f32 as the kernel implies).  A shape the launcher refuses comes back as DH_ERR_ARG with its message, nothing launched.
extern "C" int dh_dbg_conv_small(int dtype, int bwd, const void* x, int x_is_f32, const float* w, const float* bias, void* y,
                                 int y_is_f32, int accumulate, int B, int H, int W, int Cin, int Cout, void* stream) {
  DH_REQUIRE(x && w && y && B > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0, "bad arguments");
  DH_REQUIRE(x_is_f32 ? (!y_is_f32 && Cin <= 8) : y_is_f32 != 0, "few-in: f32 -> 16-bit, Cin <= 8; few-out: 16-bit -> f32");
  set_error("");
  if (bwd) launch_conv_small_bwd(dtype, x, x_is_f32, w, y, y_is_f32, accumulate, B, H, W, Cin, Cout, (hipStream_t)stream);
  else launch_conv_small_fwd(dtype, x, x_is_f32, w, bias, y, y_is_f32, B, H, W, Cin, Cout, (hipStream_t)stream);
  if (dh_last_error()[0]) return DH_ERR_ARG;
  DH_LAUNCH_CHECK();
  return DH_OK;
}
// dh_dbg_groupnorm with the backward's split form: out0 != NULL sends columns [0, split_c) of the gradient to out0 (row pitch
// split_c) and the rest to out1 (row pitch C - split_c) instead of dx (engine: the gradient of a concatenation)
extern "C" int dh_dbg_groupnorm_split(int dtype, const void* x, const float* gamma, const float* beta, void* y, float* stats,
                                      const void* dy, void* dx, float* scratch, int B, int HW, int C, int G, float eps, int silu,
                                      int accumulate, void* out0, void* out1, int split_c, void* stream) {
  DH_REQUIRE(x && y && stats && dy && dx && scratch && (!out0 || (out1 && split_c > 0 && split_c < C && split_c % 8 == 0)), "bad arguments");
  launch_groupnorm_fwd(dtype, x, gamma, beta, y, stats, scratch, B, HW, C, G, eps, silu, (hipStream_t)stream);
  GnBwdSplit split;
  split.out0 = out0; split.out1 = out1; split.split_c = split_c;
  launch_groupnorm_bwd(dtype, x, dy, gamma, beta, stats, dx, scratch, B, HW, C, G, silu, accumulate, (hipStream_t)stream, 0, split);
  DH_LAUNCH_CHECK();
  return DH_OK;
}
extern "C" int dh_dbg_gelu(int dtype, const void* x, void* y, size_t n, void* stream) {
  DH_REQUIRE(x && y && n % 8 == 0, "bad arguments (n % 8)");
  launch_gelu(dtype, x, y, n, (hipStream_t)stream);
  DH_LAUNCH_CHECK();
  return DH_OK;
}
extern "C" int dh_dbg_copy_cols(int dtype, const void* src, long lds, void* dst, long ldd, int rows, int cols, int accumulate,
                                void* stream) {
  DH_REQUIRE(src && dst && cols % 8 == 0 && lds % 8 == 0 && ldd % 8 == 0, "bad arguments (cols, pitches % 8)");
  launch_copy_cols(dtype, src, lds, dst, ldd, rows, cols, accumulate, (hipStream_t)stream);
  DH_LAUNCH_CHECK();
  return DH_OK;
}
extern "C" int dh_dbg_split_cols(int dtype, const void* src, long lds, void* dstA, long ldA, int colsA, int accA, void* dstB, long ldB,
                                 int colsB, int accB, int rows, void* stream) {
  DH_REQUIRE(src && dstA && dstB && colsA % 8 == 0 && colsB % 8 == 0 && lds % 8 == 0 && ldA % 8 == 0 && ldB % 8 == 0,
             "bad arguments (cols, pitches % 8)");
  launch_split_cols(dtype, src, lds, dstA, ldA, colsA, accA, dstB, ldB, colsB, accB, rows, (hipStream_t)stream);
  DH_LAUNCH_CHECK();
  return DH_OK;
}
// to_f32 = 0: dst (16-bit) = src (f32); to_f32 = 1: dst (f32) (=|+=) src (16-bit)
extern "C" int dh_dbg_convert(int dtype, int to_f32, const void* src, void* dst, size_t n, int accumulate, void* stream) {
  DH_REQUIRE(src && dst && (to_f32 || !accumulate), "bad arguments (only the conversion to f32 accumulates)");
  if (to_f32) launch_t_to_f32(dtype, src, (float*)dst, n, accumulate, (hipStream_t)stream);
  else launch_f32_to_t(dtype, (const float*)src, dst, n, (hipStream_t)stream);
  DH_LAUNCH_CHECK();
  return DH_OK;
}
// out [B][dim] = [cos(t f_i) | sin(t f_i)] of the one timestep at t_dev
extern "C" int dh_dbg_timestep(int dtype, const float* t_dev, int dim, int B, void* out, void* stream) {
  DH_REQUIRE(t_dev && out && dim > 0 && dim % 2 == 0 && B > 0, "bad arguments");
  launch_timestep_embedding(dtype, t_dev, dim, B, out, (hipStream_t)stream);
  DH_LAUNCH_CHECK();
  return DH_OK;
}
