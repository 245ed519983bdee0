// Kernel-side argument block and MFMA wrappers shared by the GEMM translation units (gemm.hip: k_gemm_dma, the tile families of
// rounds 1-4; gemm_pp.hip: k_gemm_pp, the eight-wave ping-pong main loop of round 5 for grids that fill the chip).
#pragma once
#include "unet_kernels.h"

namespace dh {

typedef _Float16 v8h __attribute__((ext_vector_type(8)));
typedef __bf16 v8b __attribute__((ext_vector_type(8)));
typedef float v16f __attribute__((ext_vector_type(16)));

template <class T> struct Mfma;
template <> struct Mfma<f16> {
  static __device__ __forceinline__ v16f run(uint4 a, uint4 b, v16f c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(v8h, a), __builtin_bit_cast(v8h, b), c, 0, 0, 0);
  }
};
template <> struct Mfma<bf16> {
  static __device__ __forceinline__ v16f run(uint4 a, uint4 b, v16f c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(v8b, a), __builtin_bit_cast(v8b, b), c, 0, 0, 0);
  }
};

struct GemmK {   // kernel-side copy of GemmArgs (plain data)
  const void* A; long lda;
  const void* W;
  int M, N, K;
  int mode, Hin, Win, Cin, Hout, Wout, stride, up, pad;
  const float* bias;
  const float* rowvec; int rowvec_ld; int rows_per_batch; float inv_rows_per_batch;
  const void* R; long ldr;
  void* C; long ldc;
  int act_silu;
  int pre_r;        // fetch the residual tile before the K loop
  int wide_store;   // 16-byte epilogue stores (N % 32 == 0, C and ldc 16-byte aligned)
#ifdef DH_TUNING
  int w_nt;         // non-temporal weight DMA (measured: no gain at <= 2 row tiles, a loss beyond; tuning builds only)
  unsigned long long* ts;   // in-kernel timeline of workgroup (0,0,0), lane 0 of wave 0: s_memtime at the phase boundaries
  int lnf_abl;      // timing-only ablation of the folded LayerNorm: 1 = no sums in the K loop, 2 = no exchange, 4 = no epilogue transform
#endif
  // LayerNorm folded into this GEMM (LNF instantiations): A is the LayerNorm INPUT x, W holds W * gamma, and
  // out = rstd * (x W'^T - mean * ln_s) + ln_t with ln_s[n] = sum_k W'[n][k], ln_t[n] = sum_k beta[k] W[n][k] (+ bias);
  // the row statistics come out of the K loop and are saved to ln_stats ([M][2]: mean, rstd) for the LayerNorm backward
  const float* ln_s; const float* ln_t; float* ln_stats; float ln_eps;
  float* partial;
  int splits, k_per_split;
  float* gn_part; int gn_HW, gn_G, gn_S;      // GroupNorm slice statistics of the output (split-K reduce, or the GEMM's own epilogue: gn_epi)
  int gn_epi, gn_cpg;                         // statistics in this launch's epilogue (unsplit k_gemm_dma; 1 = forward, 2 = backward with gnb_*): gn_S = 2 per row tile of an image, gn_cpg = channels per group
  const void* gnb_x; long gnb_ldx; const float *gnb_gamma, *gnb_beta, *gnb_stats; int gnb_silu;   // backward statistics
  const void* lnb_x; long lnb_ldx; const float *lnb_gamma, *lnb_stats; const void* lnb_add; void* lnb_dx;   // LayerNorm backward on the reduce (host side only)
  void* glu_y; long glu_ldy; const void* glub_x; void* glub_dx;                                    // GEGLU epilogues (GLU instantiations)
  int glub_f;       // GLU = 2: output columns [0, glub_f) are the GEGLU's dy, [glub_f, N) take the plain epilogue (glub_tile_is_glu)
  // k_gemm_pp only (launch_gemm_pp fills them): row / column tile counts, work-item order (0 = column tile fastest, 1 = row
  // tile fastest), bytes the A / W buffer descriptors cover
  int pp_tm, pp_tn, pp_order, pp_nwork; unsigned pp_a_bytes, pp_w_bytes;
  unsigned long long* pp_ts;        // timeline stamps (measurement variants only)
  // cross-attention in the epilogue (EPI_XATTN instantiations of k_gemm_dma; xa = 1 when the dispatch took the form): the tile is q
  // of head n0 / 64 for BM queries of ONE image; xa_k / xa_v = the K / V rows of image 0 at head column 0 ([B * xa_Nk][xa_ldk]),
  // xa_o [M][xa_ldo], xa_lse [B][H][xa_Nq] in k_attn_fwd's convention; q itself goes to C only when xa_save is set
  int xa, xa_Nq, xa_Nk, xa_H, xa_save;
  const void *xa_k, *xa_v; long xa_ldk; void* xa_o; long xa_ldo; float* xa_lse;
  // ... and its backward to q (EPI_XATTN_DQ, xa = 2): the tile is dO; xa_q / xa_o / xa_lse are the saved forward tensors (read),
  // xa_dq [M][xa_lddq] receives dq; C is not written
  const void* xa_q; long xa_ldq; void* xa_dq; long xa_lddq;
};


// gemm_pp.hip: the eight-wave ping-pong kernel.  gemm_pp_plan (below): whether the shape / epilogue can run on it and the policy
// wants it (GemmHooks::pp_force: test hook -- 0 policy, 1 never, 2 whenever the kernel can carry the launch); launch_gemm_pp
// launches it (the caller has filled k.splits / k.k_per_split for the tile it reports through bm / bn).
// The column-split GEGLU backward (GemmArgs::glub_f): which epilogue a column tile takes, and which tile widths can carry the
// split -- one predicate for the dispatch (host) and the kernel (device).  A tile lies wholly on one side of the seam.
__host__ __device__ constexpr bool glub_tile_is_glu(int n0, int glub_f) { return n0 < glub_f; }
__host__ __device__ constexpr bool glub_split_ok(int BN, int glub_f) { return BN > 0 && glub_f % BN == 0; }

// Cross-attention in the epilogue of the q projection (GemmArgs::xa_o), and its dQ in the epilogue of the to_out input-gradient GEMM
// (GemmArgs::xa_dq): the epilogue form numbers (the GLU template argument of
// k_gemm_dma carries it), the key rows the form stages (three 32-key blocks: the 77 text tokens), and which tiles compile / may be
// asked for it -- a 64-column tile is one head, each of its 32-row blocks one wave's queries.  One predicate for dispatch and kernel.
constexpr int EPI_XATTN = 3, EPI_XATTN_DQ = 4;
constexpr int XA_KEYS = 96;
__host__ __device__ constexpr bool xattn_epi_tile(int BM, int BN, int WG, int MW, bool BUF) {
  return BN == 64 && (BM == 64 || BM == 128) && WG == 1 && MW == 1 && BUF;
}

// ---- the host-side plan of one launch (gemm.hip: gemm_plan decides, launch_planned launches; DESIGN.md, "GEMM plan") --------------
// Everything the decision reads besides the launch itself: the test hooks, which carry-outs the caller can take, the CU count.
struct GemmHooks {
  int pp_force = 0;       // dh_dbg_gemm_family: 0 policy, 1 never k_gemm_pp, 2 k_gemm_pp whenever it can carry the launch
  int pp_glu = -1;        // dh_dbg_gemm_pp_glu: the GEGLU epilogues on k_gemm_pp (-1 policy, 0 never, 1 always)
  int pp_persist = 1;     // dh_dbg_gemm_pp_persist: 0 = one k_gemm_pp workgroup per work item
  int buf_stage = 1;      // dh_dbg_gemm_stage (bit 0 buffer staging; bits 2-5 switch the epilogue forms OFF)
  int cus = 256;          // compute units (pp_device_cus; 256 = the MI355X, and the value without a device)
  bool gn_done = false, lnb_done = false, xa_done = false;      // the caller passed GemmArgs::gn_done / lnb_done / xa_done
};
void gemm_pp_hooks(GemmHooks* h);       // gemm_pp.hip: fills pp_glu, pp_persist and cus (the one place that asks the device)

enum { RED_NONE = 0, RED_PLAIN = 1, RED_GN_FWD = 2, RED_GN_BWD = 3, RED_LN_BWD = 4 };      // the launch after a split-K GEMM
constexpr int GEMM_PLAN_FIELDS = 23;    // dh_dbg_gemm_plan writes the fields below in this order, one int32 each
struct GemmPlan {
  // which kernel
  int pp;                               // 1 = k_gemm_pp (tile bm x bn; stages .. mw are 0), 0 = k_gemm_dma
  int bm, bn, stages, wg, kg, mw;       // the k_gemm_dma tile = the template arguments of launch_tile
  int gm;                               // GM_DENSE / GM_CONV_S1 / GM_GENERIC
  int buf, lnf, epi;                    // BUF form, folded LayerNorm, epilogue form (0, GLU 1 / 2, EPI_XATTN, EPI_XATTN_DQ)
  // how it is cut
  int splits, k_per_split; unsigned grid[3];
  unsigned a_bytes, w_bytes;            // descriptor extents (0 = address form)
  // what rides along
  int gn_epi, gn_cpg, gn_S, xa;         // GroupNorm statistics (1 fwd / 2 bwd in the epilogue; gn_S: slices of the epilogue or the reduce), cross-attention (1 fwd / 2 dQ)
  int reduce;                           // RED_*
};
GemmPlan gemm_plan(const GemmK& k, size_t partial_elems, const GemmHooks& h);

// bytes the A buffer descriptor must cover (dense rows; a convolution: the whole source tensor); 0 = no whole images
inline size_t gemm_a_bytes(const GemmK& k) {
  if (k.mode == A_DENSE) return ((size_t)(k.M - 1) * k.lda + k.K) * 2;
  if (k.Hout <= 0 || k.Wout <= 0 || k.M % (k.Hout * k.Wout) != 0) return 0;
  return (size_t)(k.M / (k.Hout * k.Wout)) * k.Hin * k.Win * (size_t)k.lda * 2;
}
// a K split count: at most by_k (K tiles per split), at most `most`, no more f32 slabs than the workspace holds, at least 1
inline int clamp_splits(int splits, int by_k, int most, const GemmK& k, size_t partial_elems) {
  if (splits > by_k) splits = by_k;
  if (splits > most) splits = most;
  const size_t fit = partial_elems / ((size_t)k.M * k.N);
  if ((size_t)splits > fit) splits = (int)fit;
  return splits < 1 ? 1 : splits;
}

struct PpPlan { int bm = 0, bn = 0, splits = 1; unsigned grid = 0; };      // grid: workgroups (persistent: one per CU at most)
bool gemm_pp_plan(const GemmK& k, size_t partial_elems, const GemmHooks& h, PpPlan* plan);
void launch_gemm_pp(int dtype, const GemmK& k, const PpPlan& plan, hipStream_t st, hipEvent_t e0, hipEvent_t e1);

}  // namespace dh
