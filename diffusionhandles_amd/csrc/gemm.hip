// MFMA implicit-GEMM for gfx950:  D[m][n] = sum_k A(m,k) * W[n][k]  (+ epilogue)
//
//   A(m,k): dense rows, or the im2col view of a channels-last image for a 3x3 convolution
//           (stride 1/2, optional nearest-2x upsampled source), or the transposed-stride-2
//           view used by the input-gradient of a stride-2 convolution.  K is ordered
//           (64-channel chunk, tap, channel in chunk) -- conv_k_index -- so a 64-wide K tile lies inside
//           one tap (the gather is a row of 64 contiguous channels of a shifted pixel, zero outside the
//           image) and the nine taps of a chunk follow each other while its rows are in the L2.
//   W:      [N][K] with K contiguous (torch Linear layout; conv weights are re-laid to
//           [Cout][Cin/64][ky][kx][64] at load time).
//
// 256 threads = 4 waves (2 x 2) per wave group.  Per K tile of 64: LDS-DMA (global_load_lds_dwordx4) into a ring of
// unpadded, source-swizzled stages (see k_gemm_dma below) -> ds_read_b128 fragments ->
// v_mfma_f32_32x32x16 with the operands SWAPPED (W is the A operand), so a lane owns one
// output row m and 4 consecutive n per accumulator group: 8-byte stores, per-lane row
// scalars.  f32 accumulate; optional split-K through f32 partial slabs + a reduce kernel
// that applies the same epilogue (and, when a GroupNorm follows, leaves its slice statistics).
// Round 6: the LDS-DMA of the dense and stride-1 3x3 forms goes through buffer descriptors (BUF instantiations: scalar K cursor /
// tap offset, hardware zero fill; bit-identical to the address form, tools/fuzz_gemm_stage.py), and an UNSPLIT launch whose output a
// GroupNorm consumes leaves that GroupNorm's slice statistics from its own epilogue (gn_epi = 1), as does an unsplit input-gradient
// launch whose output is dy of a GroupNorm for that GroupNorm's BACKWARD statistics (gn_epi = 2; tools/fuzz_gn_epilogue.py).
#include <stdlib.h>

#include <string.h>

#include <type_traits>
#include <vector>

#include <hip/hip_ext.h>

#include "attn_tile.h"
#include "gemm_k.h"

namespace dh {

// optional HIP-event bracket around every k_gemm launch (bench.py roofline measurement)
struct GemmProf {
  bool on = false;
  std::vector<hipEvent_t> ev;
  size_t used = 0;
  double flops = 0;
  double bytes = 0;                           // algorithmic HBM bytes of the bracketed launches (see dh_gemm_profile_bytes)
  hipEvent_t e0 = nullptr, e1 = nullptr;      // start / stop events of the launch being issued (hipExtLaunchKernelGGL)
};
static GemmProf g_prof;
static int g_buf_stage = 1;     // test hook (dh_dbg_gemm_stage): 0 = the address form of rounds 1-5 everywhere
static int g_pp_force = 0;      // test hook (dh_dbg_gemm_family): 0 = policy, 1 = never k_gemm_pp, 2 = k_gemm_pp whenever it can carry the launch
// the plan of this thread's last launch (test hooks dh_dbg_gemm_last_tile, dh_dbg_gemm_xattn_carried): written by launch_gemm after the
// launch, never read by the planning
static thread_local GemmPlan g_last_plan;
// ... and the tile that launch really instantiated, written by launch_tile from its own template arguments (k_gemm_pp: bm, bn only):
// dh_dbg_gemm_last_tile reports these, so a test that compares them with the plan sees a wrong arm of launch_planned's switch
struct LaunchedTile { int bm, bn, kg, stages, mw; };
static thread_local LaunchedTile g_launched_tile;
static thread_local long long g_xattn_total = 0;    // how many launches of this thread have carried a cross-attention in their epilogue
#ifdef DH_TUNING
static unsigned long long* g_gemm_ts = nullptr;      // device buffer of 8 stamps (dh_dbg_gemm_timeline)
#endif
bool gemm_profiling_on() { return g_prof.on; }

constexpr int BK = 64;
// experiment switches (tools/lab.sh build-tuning DH_DEFS=...): never defined in the product build
#ifdef DH_EXP_SETPRIO
#define DH_PRIO(x) __builtin_amdgcn_s_setprio(x)
#else
#define DH_PRIO(x) do { } while (0)
#endif


// bias / per-image vector / SiLU / residual of four consecutive outputs of row m, rounded to the storage type
template <class T>
__device__ __forceinline__ uint2 epilogue_pack(const GemmK& p, int m, int n, float v0, float v1, float v2, float v3,
                                               bool have_r, uint2 rpre, bool have_b, float4 bpre) {
  float v[4] = {v0, v1, v2, v3};
  if (p.bias) {
    float4 b = bpre;        // (not `have_b ? bpre : *ptr`: a conditional of two lvalues selects an ADDRESS, which puts bpre on the stack)
    if (!have_b) b = *reinterpret_cast<const float4*>(p.bias + n);
    v[0] += b.x; v[1] += b.y; v[2] += b.z; v[3] += b.w;
  }
  if (p.rowvec) {
    const float4 b = *reinterpret_cast<const float4*>(p.rowvec + (size_t)div_small(m, p.inv_rows_per_batch) * p.rowvec_ld + n);
    v[0] += b.x; v[1] += b.y; v[2] += b.z; v[3] += b.w;
  }
  if (p.act_silu) {
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = v[i] / (1.f + __expf(-v[i]));
  }
  typedef T T4 __attribute__((ext_vector_type(4)));      // register-only views: an address-taken local costs a scratch slot
  if (p.R) {
    const T* r = reinterpret_cast<const T*>(p.R) + (size_t)m * p.ldr + n;
    uint2 raw = rpre;
    if (!have_r) raw = *reinterpret_cast<const uint2*>(r);
    const T4 rv = __builtin_bit_cast(T4, raw);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] += to_f32<T>(rv[i]);
  }
  T4 o;
#pragma unroll
  for (int i = 0; i < 4; ++i) o[i] = from_f32<T>(v[i]);
  return __builtin_bit_cast(uint2, o);
}
template <class T>
__device__ __forceinline__ void epilogue_store(const GemmK& p, int m, int n, float v0, float v1, float v2, float v3,
                                               bool have_r = false, uint2 rpre = make_uint2(0, 0), bool have_b = false,
                                               float4 bpre = make_float4(0.f, 0.f, 0.f, 0.f)) {
  *reinterpret_cast<uint2*>(reinterpret_cast<T*>(p.C) + (size_t)m * p.ldc + n) =
      epilogue_pack<T>(p, m, n, v0, v1, v2, v3, have_r, rpre, have_b, bpre);
}

// the same epilogue for one element (used for the GroupNorm pivots of k_splitk_reduce_gn)
template <class T>
__device__ __forceinline__ float epilogue_scalar(const GemmK& p, int m, int n, float v) {
  if (p.bias) v += p.bias[n];
  if (p.rowvec) v += p.rowvec[(size_t)div_small(m, p.inv_rows_per_batch) * p.rowvec_ld + n];
  if (p.act_silu) v = v / (1.f + __expf(-v));
  if (p.R) v += to_f32<T>(reinterpret_cast<const T*>(p.R)[(size_t)m * p.ldr + n]);
  return to_f32<T>(from_f32<T>(v));
}

// ---------------------------------------------------------------------------------------------
// LDS-DMA variant: global_load_lds_dwordx4 fills a ring of ST stages directly (no staging
// registers), so ST-1 K tiles are in flight per workgroup while tile t is multiplied.
//   * stage image: A rows then W rows, 128 B per row, UNPADDED (the DMA destination is
//     wave-uniform base + lane*16); bank conflicts are avoided by an XOR swizzle applied on the
//     per-lane SOURCE address (16-byte chunk c of row r is stored at chunk c ^ ((r >> 1) & 7): gfx950's
//     ds_read_b128 serves 16 lanes per cycle from a 256-byte bank row = TWO 128-byte tile rows, and its lane
//     groups {0-3,12-15,20-27} / {4-11,16-19,28-31} then hit 16 distinct 16-byte slots) and
//     undone on the fragment read.
//   * the DMA is issued from inline asm (m0 = LDS destination), so hipcc does not see a pending
//     LDS write and does not drain vmcnt(0) in front of every ds_read; ordering is by hand:
//     counted s_waitcnt vmcnt(N) -> s_barrier -> ds_read of the landed stage.
//   * rows outside the matrix / the image read from a 128-byte zero page instead.
__device__ uint4 g_zero_page[8];

__device__ __forceinline__ void dma16(const void* gsrc, unsigned lds_dst) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}

// the same with the non-temporal hint: weight tiles that only one or two workgroups read (small M) stream through
// without displacing the activations / code / kernel arguments that the next kernels re-read from L2 and MALL
__device__ __forceinline__ void dma16_nt(const void* gsrc, unsigned lds_dst) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off nt\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}

// LDS-DMA through a buffer descriptor (BUF instantiations; the form of gemm_pp.hip pp_dma): M0 = LDS destination of the piece (not
// saved: nothing else in these kernels reads M0 -- LDS instructions need none on gfx9+, tests/test_abi.py audits the ISA), the
// scalar offset copied by an s_mov inside the statement (MUBUF's soffset must be an SGPR; a VALU-written SGPR -- v_readfirstlane --
// must not be read by a VMEM instruction for five wait states and hipcc pads nothing for asm operands; the copy also is the wait
// state M0 needs in front of the DMA).
typedef int buf_v4i __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void buf_dma16(unsigned voff, buf_v4i rsrc, unsigned soff, unsigned lds_dst) {
  unsigned tmp;
  soff = __builtin_amdgcn_readfirstlane(soff);
  lds_dst = __builtin_amdgcn_readfirstlane(lds_dst);
  asm volatile("s_mov_b32 m0, %4\n\ts_mov_b32 %0, %3\n\tbuffer_load_dwordx4 %1, %2, %0 offen lds"
               : "=&s"(tmp) : "v"(voff), "s"(rsrc), "s"(soff), "s"(lds_dst) : "memory");
}
// voff with bit 31 set (out of range for every descriptor below 2 GiB: the DMA writes zeros) when bit (31 - sh) of nt is set
__device__ __forceinline__ unsigned buf_mask_oob(unsigned nt, unsigned sh, unsigned voff) {
  return ((nt << sh) & 0x80000000u) | voff;
}

template <int N> __device__ __forceinline__ void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

enum { GM_DENSE = 0, GM_CONV_S1 = 1, GM_GENERIC = 2 };
#ifdef DH_TUNING
#define LNF_ABL(bit) && !(p.lnf_abl & (bit))
#define LEAN_ABL && !(p.lnf_abl & 8)
#define DH_STAMP(i) do { if (p.ts && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && threadIdx.x == 0) p.ts[i] = __builtin_amdgcn_s_memtime(); } while (0)
// per-K-tile stamps of the same wave (slots 8 ..): 3 per tile -- loop top, tile landed + barrier passed, multiplies and next issue done
#define DH_STAMP_T(kt, j) do { if (p.ts && (kt) < 40 && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && threadIdx.x == 0) p.ts[8 + 3 * (kt) + (j)] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define DH_STAMP_T(kt, j) do { } while (0)
#define LNF_ABL(bit)
#define LEAN_ABL
#define DH_STAMP(i) do { } while (0)
#endif

// sum and sum of squares of the 8 16-bit values of an MFMA operand fragment (f32 accumulate, v_dot2c)
typedef _Float16 v2h __attribute__((ext_vector_type(2)));
typedef __bf16 v2b __attribute__((ext_vector_type(2)));
typedef unsigned u4v __attribute__((ext_vector_type(4)));
template <class T> __device__ __forceinline__ void frag_sums(const uint4& f, float& s1, float& s2);
// (the empty asm pins the fragment as ONE 128-bit register tuple: without it the compiler scalarises the uint4, re-groups
// the LDS reads of the A fragments into ds_read_b96 + ds_read2st64_b32 pieces, and those break the conflict-free
// ds_read_b128 pattern the tile swizzle is built for)
template <> __device__ __forceinline__ void frag_sums<f16>(const uint4& f_in, float& s1, float& s2) {
  const v2h one = {(_Float16)1.f, (_Float16)1.f};
  u4v f = __builtin_bit_cast(u4v, f_in);
  asm("" : "+v"(f));
  const unsigned w[4] = {f[0], f[1], f[2], f[3]};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const v2h h = __builtin_bit_cast(v2h, w[i]);
    s1 = __builtin_amdgcn_fdot2(h, one, s1, false);
    s2 = __builtin_amdgcn_fdot2(h, h, s2, false);
  }
}
template <> __device__ __forceinline__ void frag_sums<bf16>(const uint4& f_in, float& s1, float& s2) {
  const v2b one = {(__bf16)1.f, (__bf16)1.f};
  u4v f = __builtin_bit_cast(u4v, f_in);
  asm("" : "+v"(f));
  const unsigned w[4] = {f[0], f[1], f[2], f[3]};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const v2b h = __builtin_bit_cast(v2b, w[i]);
    s1 = __builtin_amdgcn_fdot2_f32_bf16(h, one, s1, false);
    s2 = __builtin_amdgcn_fdot2_f32_bf16(h, h, s2, false);
  }
}

// WG = 2: two groups of four waves share every staged tile; group g multiplies k-steps [g, g+1) * KK/2 of it and
// issues half of the DMA pieces, and the groups' accumulators are added through LDS before the epilogue.  Same
// LDS and DMA traffic as WG = 1 but two waves per SIMD, so one wave's ds_read / barrier waits sit under the
// other's MFMAs (a single image fills the chip with at most one 4-wave block per CU).
// KG > 1: KG groups of four waves with a ring each work on DISJOINT K ranges of the block's tile (split-K inside
// the workgroup): a GEMM with few output tiles and a long K loop is bounded by the serial depth of that loop
// (~0.6 us per K tile), and this divides the depth by KG without partial slabs in HBM or a reduce launch.
// MW = 2: eight waves laid out 4 (M) x 2 (N) over a 256-row tile, 64 x (BN/2) outputs per wave as before: the A and W
// tiles are shared by twice the MFMA work, so the staging traffic per flop (the TA / LDS-DMA issue that bounds the
// 4-wave kernel on big grids) drops by a quarter and two waves share every SIMD.  For grids that fill the machine.
// GLU = 1: the tile is the (paired-layout) pre-activation of a GEGLU: the epilogue also writes h * gelu(gate) (and the
// pre-activations only when p.C is set); GLU = 2: the tile is dy of a GEGLU: the epilogue reads the saved pre-activations of its
// rows and writes d_value / d_gate instead of dy.  Both keep the activation where the data already sits in registers
// (reference model/attention.py:345-400; diffusers GEGLU [ext]).
// GLU = EPI_XATTN (3): the tile is q of one cross-attention head (64 columns) for BM queries of one image: the epilogue runs that
// head's attention over its (at most XA_KEYS) text keys and writes o and lse; q goes to memory only for a backward pass.  The
// 16-bit q tile crosses the two wave columns through the idle rings, K and V ride under the K loop in registers like the residual.
// GLU = EPI_XATTN_DQ (4): the tile is dO of one cross-attention head (the input-gradient GEMM of attn2.to_out.0): the epilogue forms
// dq of its queries from the saved q, o, lse and the head's K / V (k_attn_bwd_dq's products) and writes dq; dO is not written.
// BUF (round 6): the staging of k_gemm_pp under this kernel's loop -- the LDS-DMA goes through a buffer descriptor
// (`buffer_load_dwordx4 ... lds`): one 32-bit lane offset per piece computed once, the K cursor / the 3x3 tap in the scalar
// offset, rows past M and taps outside the image = an out-of-range offset that the hardware turns into zeros (no zero page, no
// 64-bit address arithmetic, no select pair, no M0 save / restore per piece).  Dense and stride-1 3x3 operands; the generic
// gather (stride 2, up-sampled source, transposed stride 2) keeps the address form.
// Which k_gemm_dma tiles leave GroupNorm slice statistics in their epilogue: the forward form (gn_epi 1: two wave columns, at most
// 128 columns, the plain epilogue) and the backward form (gn_epi 2: 64-column tiles of at most 128 rows, one wave group).  The
// dispatch asks for a form only where these hold, and the kernel compiles the form only where they hold: one predicate for both.
constexpr bool gn_epi_fwd_tile(int BN, int GLU, bool LNF) { return GLU == 0 && !LNF && BN % 64 == 0 && BN <= 128; }
constexpr bool gn_epi_bwd_tile(int BM, int BN, int WG, int GLU, bool LNF) {
  return gn_epi_fwd_tile(BN, GLU, LNF) && BN == 64 && BM <= 128 && WG == 1;
}

template <class T, int BM, int BN, int ST, int MODE, int ABL = 0, int WG = 1, int KG = 1, int MW = 1, bool LNF = false, int GLU = 0, bool BUF = false>   // ABL: diagnostics (1 = no LDS reads/MFMA, 2 = no DMA in the loop)
__global__ void __launch_bounds__(256 * WG * KG * MW) k_gemm_dma(const GemmK p) {
  static_assert(!BUF || MODE != GM_GENERIC, "the generic gather stages through addresses");
  static_assert((WG == 1) + (KG == 1) + (MW == 1) >= 2, "one kind of wave grouping per instantiation");
  static_assert(!LNF || (WG == 1 && MODE == GM_DENSE), "the folded LayerNorm needs every k-step of a row in one wave group");
  DH_STAMP(0);
  constexpr int NWV = 4 * MW;                               // waves that share one staged tile
  // wave arrangement: two wave columns (each wave BN / 2 columns), or ONE when BN is not a multiple of 64 -- the 128x160
  // tile: four wave rows of 32 x 160 outputs (1 x 5 blocks of 32 x 32 per wave, the wave shape of the eight-wave 128x320 tile)
  constexpr int WNS = BN % 64 ? 1 : 2, WMS = NWV / WNS;
  constexpr int RPW = BM / WMS, CPW = BN / WNS;             // rows / columns of the output tile per wave
  constexpr int TM = RPW / 32, TN = CPW / 32;
  static_assert(RPW % 32 == 0 && CPW % 32 == 0, "a wave owns whole 32 x 32 blocks");
  static_assert(WNS == 2 || (!LNF && GLU == 0 && WG == 1 && KG == 1), "the one-column arrangement carries the plain epilogue only");
  constexpr int NPA = BM / 32 / WG / MW, NPB = BN / 32 / WG / MW;     // 1-KiB pieces per wave per stage
  constexpr int NP = NPA + NPB;
  constexpr int STAGE = (BM + BN) * 128;
  __shared__ __attribute__((aligned(1024))) unsigned char smem_all[KG * ST * STAGE];

  const int tid = threadIdx.x, lane = tid & 63, wave = (tid >> 6) & (NWV - 1);
  const int grp = WG > 1 ? __builtin_amdgcn_readfirstlane(tid >> 8) : 0;     // wave-uniform (feeds m0 through dma16)
  const int kg = KG > 1 ? __builtin_amdgcn_readfirstlane(tid >> 8) : 0;
  unsigned char* smem = smem_all + kg * (ST * STAGE);
  const int wm = WNS == 2 ? wave >> 1 : wave, wn = WNS == 2 ? wave & 1 : 0, ln = lane & 31, hi = lane >> 5;
  const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
  int kbeg = blockIdx.z * p.k_per_split;
  int kend = kbeg + p.k_per_split;
  if (kend > p.K) kend = p.K;
  int ntiles = (kend - kbeg) / BK;
  int loop_tiles = ntiles;                          // trip count of the K loop (uniform over the block: barriers)
  if (KG > 1) {
    loop_tiles = (ntiles + KG - 1) / KG;
    kbeg += kg * loop_tiles * BK;
    ntiles -= kg * loop_tiles;
    ntiles = ntiles < 0 ? 0 : (ntiles > loop_tiles ? loop_tiles : ntiles);
  }
  const T* Ag = reinterpret_cast<const T*>(p.A);
  const int wave_s = __builtin_amdgcn_readfirstlane(wave);      // scalar copy: the DMA destinations are scalar arithmetic
  const unsigned lds0 = (unsigned)(size_t)((__attribute__((address_space(3))) unsigned char*)smem_all) + kg * (ST * STAGE);
  const int prow = lane >> 3;                       // row of this lane inside a piece
  // logical chunk this lane fetches (swizzle on the source): piece rows are 8 (wave + 4 j) + prow, so ((row >> 1) & 7)
  const int lchunk = (lane & 7) ^ (4 * (wave & 1) + (prow >> 1));
  const T* zero = reinterpret_cast<const T*>(g_zero_page) + (lane & 7) * 8;

  // A rows of this lane: one per piece
  const float inv_hw = MODE == GM_DENSE ? 0.f : __builtin_amdgcn_rcpf((float)(p.Hout * p.Wout));
  const float inv_w = MODE == GM_DENSE ? 0.f : __builtin_amdgcn_rcpf((float)p.Wout);
  bool a_ok[NPA];
  long a_off[NPA];      // dense: row offset; conv: offset of the (centre / first) source pixel or batch base
  int a_oy[NPA], a_ox[NPA];
#pragma unroll
  for (int j = 0; j < NPA; ++j) {
    const int m = m0 + 8 * (wave + NWV * (j * WG + grp)) + prow;
    a_ok[j] = m < p.M;
    if (MODE == GM_DENSE) {
      // rows past M read row M - 1 again (their products are never stored): no select in the loop
      a_off[j] = (long)(a_ok[j] ? m : p.M - 1) * p.lda + lchunk * 8;
      a_oy[j] = a_ox[j] = 0;
    } else {
      const int hw = p.Hout * p.Wout;
      const int b = div_small(m, inv_hw), r = m - b * hw;
      a_oy[j] = div_small(r, inv_w);
      a_ox[j] = r - a_oy[j] * p.Wout;
      if (MODE == GM_CONV_S1) a_off[j] = (((long)b * p.Hin + a_oy[j]) * p.Win + a_ox[j]) * p.lda + lchunk * 8;
      else a_off[j] = (long)b * p.Hin * p.Win;
    }
  }
  // stride-1 3x3: which of the nine taps of this lane's pixel lie inside the image (bit = tap), decided once
  unsigned a_taps[NPA];
#pragma unroll
  for (int j = 0; j < NPA; ++j) {
    a_taps[j] = 0;
    if (MODE == GM_CONV_S1 && a_ok[j]) {
#pragma unroll
      for (int t = 0; t < 9; ++t)
        if ((unsigned)(a_oy[j] + t / 3 - 1) < (unsigned)p.Hin && (unsigned)(a_ox[j] + t % 3 - 1) < (unsigned)p.Win) a_taps[j] |= 1u << t;
    }
  }
  // W pieces: contiguous 1 KiB blocks of the tiled layout (rows 8*(wave+4j).. of the BN-row tile)
  const T* Wg = reinterpret_cast<const T*>(p.W);
  const int KT = p.K >> 6;
  const T* b_ptr[NPB];
#pragma unroll
  for (int j = 0; j < NPB; ++j) {
    const int row = 8 * (wave + NWV * (j * WG + grp));     // first row of the piece inside the BN tile
    b_ptr[j] = Wg + ((size_t)((n0 + row) >> 6) * KT) * 4096 + (size_t)((n0 + row) & 63) * 64 + lane * 8;     // (n0 % 64 = 32 on odd 160-column tiles)
  }
  int tap = 0, c0 = 0;
  if (MODE != GM_DENSE) { const int kt0 = kbeg >> 6, ch = kt0 / 9; tap = kt0 - ch * 9; c0 = ch * BK; }    // conv_k_index order
  // BUF: descriptors (scalar), one 32-bit source offset per A piece, one scalar offset per W piece.  The A base is moved back by
  // one image row + one pixel (a_bias) so that the tap offset (ky Win + kx) lda in the scalar offset is never negative.
  typedef int bv4i __attribute__((ext_vector_type(4)));
  bv4i ra = {0, 0, 0, 0}, rw = {0, 0, 0, 0};
  unsigned bv_a[NPA], bv_nt[NPA], bs_w[NPB];
  unsigned bs_tap = 0, bs_sh = 0;                     // conv: scalar offset and validity shift of the tile at the issue cursor
  unsigned bs_step_px = 0, bs_step_row = 0; int bs_kx = 0;
  const unsigned bv_w = lane * 16;
  if constexpr (BUF) {
    const unsigned a_bias = MODE == GM_CONV_S1 ? (unsigned)((p.Win + 1) * (int)p.lda * 2) : 0u;
    const size_t a_base = (size_t)p.A - a_bias;
    ra[0] = (int)(unsigned)a_base; ra[1] = (int)((a_base >> 32) & 0xffff); ra[2] = (int)(p.pp_a_bytes + a_bias); ra[3] = 0x00020000;
    rw[0] = (int)(unsigned)(size_t)p.W; rw[1] = (int)(((size_t)p.W >> 32) & 0xffff); rw[2] = (int)p.pp_w_bytes; rw[3] = 0x00020000;
#pragma unroll
    for (int j = 0; j < NPA; ++j) {
      const int m = m0 + 8 * (wave + NWV * (j * WG + grp)) + prow;
      if (MODE == GM_DENSE) {
        bv_a[j] = a_ok[j] ? (unsigned)m * (unsigned)((int)p.lda * 2) + (unsigned)lchunk * 16u : 0x80000000u;
        bv_nt[j] = 0;
      } else {
        const int hw = p.Hout * p.Wout;
        const int b = div_small(m, inv_hw);
        (void)hw;
        bv_a[j] = (unsigned)((b * p.Hin + a_oy[j]) * p.Win + a_ox[j]) * (unsigned)((int)p.lda * 2) + (unsigned)lchunk * 16u;
        bv_nt[j] = ~a_taps[j];                        // bit t set: tap t of this lane's pixel lies outside the image (or the row is past M)
      }
    }
#pragma unroll
    for (int j = 0; j < NPB; ++j) {
      const int n = n0 + 8 * (wave_s + NWV * (j * WG + grp));
      bs_w[j] = (unsigned)(((n >> 6) * KT) * 8192 + (n & 63) * 128);
    }
    if (MODE == GM_CONV_S1) {
      const int ky = tap / 3, kx = tap - ky * 3;
      bs_tap = (unsigned)((ky * p.Win + kx) * (int)p.lda + c0) * 2u;
      bs_sh = 31u - (unsigned)tap;
      bs_kx = kx;
      bs_step_px = (unsigned)((int)p.lda * 2);
      bs_step_row = (unsigned)((p.Win - 2) * (int)p.lda * 2);
    }
  }

  // one 1-KiB piece q (0..NPA-1: A rows, NPA..NP-1: W rows) of K tile kt into ring slot `stage`;
  // the conv (tap, c0) cursor belongs to the tile currently being issued and advances with next_tile()
  auto issue_piece = [&](int kt, int stage, int q) {
    const int k0 = kbeg + kt * BK;
    const unsigned sbase = __builtin_amdgcn_readfirstlane(lds0 + stage * STAGE + wave_s * 1024);
    if constexpr (BUF) {
      if (q < NPA) {
        const int j = q;
        const unsigned dst = sbase + (j * WG + grp) * (NWV * 1024);
        if (MODE == GM_DENSE) buf_dma16(bv_a[j], ra, (unsigned)k0 * 2u, dst);
        else buf_dma16(buf_mask_oob(bv_nt[j], bs_sh, bv_a[j]), ra, bs_tap, dst);
      } else {
        const int j = q - NPA;
        buf_dma16(bv_w, rw, bs_w[j] + (unsigned)(k0 >> 6) * 8192u, sbase + BM * 128 + (j * WG + grp) * (NWV * 1024));
      }
      return;
    }
    if (q < NPA) {
      const int j = q;
      if (MODE == GM_DENSE) {
        const T* ptr = Ag + a_off[j] + k0;
        dma16(ptr, sbase + (j * WG + grp) * (NWV * 1024));
      } else if (MODE == GM_CONV_S1) {
        const int ky = tap / 3, kx = tap - ky * 3;
        const long toff = ((long)(ky - 1) * p.Win + (kx - 1)) * p.lda + c0;
        const bool ok = (a_taps[j] & (1u << tap)) != 0;
        const T* ptr = Ag + a_off[j] + toff;
        dma16(ok ? ptr : zero, sbase + (j * WG + grp) * (NWV * 1024));
      } else {
        const int ky = tap / 3, kx = tap - ky * 3;
        bool ok = a_ok[j];
        int sy, sx;
        if (p.mode == A_CONV3) {
          const int iy = a_oy[j] * p.stride + ky - p.pad, ix = a_ox[j] * p.stride + kx - p.pad;
          ok = ok && iy >= 0 && ix >= 0 && iy < (p.Hin << p.up) && ix < (p.Win << p.up);
          sy = iy >> p.up; sx = ix >> p.up;
        } else {
          const int ty = a_oy[j] + ky - 1, tx = a_ox[j] + kx - 1;
          ok = ok && ty >= 0 && tx >= 0 && !(ty & 1) && !(tx & 1) && (ty >> 1) < p.Hin && (tx >> 1) < p.Win;
          sy = ty >> 1; sx = tx >> 1;
        }
        sy = sy < 0 ? 0 : (sy >= p.Hin ? p.Hin - 1 : sy);
        sx = sx < 0 ? 0 : (sx >= p.Win ? p.Win - 1 : sx);
        const T* ptr = Ag + (a_off[j] + (long)sy * p.Win + sx) * p.lda + c0 + lchunk * 8;
        dma16(ok ? ptr : zero, sbase + (j * WG + grp) * (NWV * 1024));
      }
    } else {
      const int j = q - NPA;
#ifdef DH_TUNING
      if (p.w_nt) dma16_nt(b_ptr[j] + (size_t)(k0 >> 6) * 4096, sbase + BM * 128 + (j * WG + grp) * (NWV * 1024));
      else
#endif
      dma16(b_ptr[j] + (size_t)(k0 >> 6) * 4096, sbase + BM * 128 + (j * WG + grp) * (NWV * 1024));
    }
  };
  auto next_tile = [&]() {
    if constexpr (BUF && MODE == GM_CONV_S1) {
      // scalar cursor: one pixel to the right, at the end of a kernel row down to the start of the next, after nine taps the next
      // 64-channel chunk (uniform selects: the offset stays in a scalar register)
      ++tap; ++bs_kx;
      const bool row_end = bs_kx == 3;
      bs_tap += row_end ? bs_step_row : bs_step_px;
      bs_kx = row_end ? 0 : bs_kx;
      if (tap == 9) { tap = 0; c0 += BK; bs_tap = (unsigned)c0 * 2u; }
      bs_sh = 31u - (unsigned)tap;
      return;
    }
    if (MODE != GM_DENSE) { if (++tap == 9) { tap = 0; c0 += BK; } }
  };
  auto issue = [&](int kt, int stage) {
#pragma unroll
    for (int q = 0; q < NP; ++q) issue_piece(kt, stage, q);
    next_tile();
  };

  v16f acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int wn_u = __builtin_amdgcn_readfirstlane(wn);       // wave-uniform copy (scalar branch in the K loop)
  float ln1[TM], ln2[TM];          // LNF: per-lane partial sum x / sum x^2 of the lane's rows (this lane's half of every k-step)
#pragma unroll
  for (int i = 0; i < TM; ++i) { ln1[i] = 0.f; ln2[i] = 0.f; }

#pragma unroll
  for (int s = 0; s < ST - 1; ++s)
    if (s < ntiles) issue(s, s);
  DH_STAMP(1);

  // the residual tile is fetched now and added in the epilogue: its cold load flies under the K loop instead of
  // sitting at the tail of the kernel (these loads are younger than the prologue DMAs and older than every later one,
  // so the counted vmcnt waits below can only become stricter)
  constexpr bool PRE = TM * TN <= 8;               // the prefetched tiles cost 8 registers per 32x32 output tile
  // (a GEGLU-backward tile of the column-split form writes no C: nothing to add there)
  const bool pre_r = PRE && p.R != nullptr && p.pre_r && p.splits == 1 && (WG == 1 || grp == 0) && (KG == 1 || kg == 0) &&
                     (GLU != 2 || !glub_tile_is_glu(n0, p.glub_f));
  // (the eight-wave 128x320 tile holds five column blocks per wave: 80 registers of prefetched bias would push it over the
  //  256-register budget of two waves per SIMD; its bias is read in the epilogue, a warm 1.3 KB vector)
  constexpr bool PRE_B = PRE && !(MW == 2 && BN == 320) && WNS == 2;
  const bool pre_b = PRE_B && p.bias != nullptr && p.pre_r && p.splits == 1;
  float4 bpre[PRE_B ? TN : 1][4];
  if (pre_b) {
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int n = n0 + wn * CPW + j * 32 + 8 * g + 4 * hi;
        bpre[PRE_B ? j : 0][g] = n < p.N ? *reinterpret_cast<const float4*>(p.bias + n) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
  }
  // folded LayerNorm: the per-column vectors are fetched under the K loop as well (their loads were the exposed tail)
  constexpr bool PRE_LN = LNF && PRE && !(MW == 2 && BM == 256);     // (the 256x128 eight-wave tile has no registers to spare: it would spill)
  float4 lsp[PRE_LN ? TN : 1][4], ltp[PRE_LN ? TN : 1][4];
  if (PRE_LN) {
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int n = n0 + wn * CPW + j * 32 + 8 * g + 4 * hi;
        lsp[PRE_LN ? j : 0][g] = n < p.N ? *reinterpret_cast<const float4*>(p.ln_s + n) : make_float4(0.f, 0.f, 0.f, 0.f);
        ltp[PRE_LN ? j : 0][g] = n < p.N ? *reinterpret_cast<const float4*>(p.ln_t + n) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
  }
  // GroupNorm BACKWARD statistics in the epilogue (p.gn_epi == 2, round 6; see the epilogue): the tile is dy of a GroupNorm whose
  // input tile x rides under the K loop in the residual's prefetch registers (the dispatch takes the form only when there is no
  // residual), and thread n of the first wave fetches (gamma, beta, mean, rstd) of tile column n for the table the epilogue
  // builds in LDS -- four registers across the loop instead of 64
  constexpr bool GNB = gn_epi_bwd_tile(BM, BN, WG, GLU, LNF);
  static_assert(!GNB || (PRE && WNS == 2), "the backward form carries the GroupNorm input tile in the residual's prefetch registers");
  const bool gnb = GNB && p.gn_epi == 2 && p.splits == 1;
  const bool pre_x = gnb && (KG == 1 || kg == 0);
  float4 gnb_col = make_float4(0.f, 0.f, 0.f, 0.f);
  if (GNB && pre_x && tid < BN) {
    const int n = n0 + tid, grp_n = (int)(((float)n + 0.5f) / (float)p.gn_cpg);
    const float2 st2 = *reinterpret_cast<const float2*>(p.gnb_stats + 2 * ((m0 / p.gn_HW) * p.gn_G + grp_n));
    gnb_col = make_float4(p.gnb_gamma[n], p.gnb_beta[n], st2.x, st2.y);
  }
  uint2 rpre[TM][TN][4];
  if (pre_r || pre_x) {
    const T* rsrc = reinterpret_cast<const T*>(pre_x ? p.gnb_x : p.R);
    const long rld = pre_x ? p.gnb_ldx : p.ldr;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int m = m0 + wm * RPW + i * 32 + ln;
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int n = n0 + wn * CPW + j * 32 + 8 * g + 4 * hi;
          rpre[i][j][g] = (m < p.M && n < p.N) ? *reinterpret_cast<const uint2*>(rsrc + (size_t)m * rld + n) : make_uint2(0, 0);
        }
    }
  }

  // cross-attention epilogue (p.xa): the head's K and V rows do not depend on this launch -- their 2 x XA_KEYS x 8 sixteen-byte
  // chunks are fetched now by the 256 threads of the first wave group and fly under the K loop (rows past Nk read the last key
  // again: finite values behind masked scores, as in attention.hip)
  constexpr bool XA = GLU == EPI_XATTN || GLU == EPI_XATTN_DQ, XB = GLU == EPI_XATTN_DQ;
  static_assert(!XB || !LNF, "the input-gradient GEMM carries no LayerNorm");
  static_assert(!XA || xattn_epi_tile(BM, BN, WG, MW, BUF), "the cross-attention epilogue lives on the buffer-staged 64x64 / 128x64 tiles");
  constexpr int XA_CH = XA_KEYS * 8 / 256;         // chunks per thread and matrix
  u4v xa_kr[XA ? XA_CH : 1], xa_vr[XA ? XA_CH : 1];      // (vector types: a struct copy from memory is a memcpy the private array does not survive as registers)
  if constexpr (XA) {
    if (KG == 1 || kg == 0) {
      const int b = div_small(m0, __builtin_amdgcn_rcpf((float)p.xa_Nq));
      const size_t head = (size_t)b * p.xa_Nk * p.xa_ldk + n0;
      const T* kp = reinterpret_cast<const T*>(p.xa_k) + head;
      const T* vp = reinterpret_cast<const T*>(p.xa_v) + head;
#pragma unroll
      for (int j = 0; j < XA_CH; ++j) {
        const int idx = tid + j * 256;
        int r = idx >> 3;
        r = r < p.xa_Nk ? r : p.xa_Nk - 1;
        const size_t off = (size_t)r * p.xa_ldk + (idx & 7) * 8;
        xa_kr[j] = *reinterpret_cast<const u4v*>(kp + off);
        xa_vr[j] = *reinterpret_cast<const u4v*>(vp + off);
      }
    }
  }
  // ... and the backward form's saved q / o rows and lse of the 32 queries this wave will own in the epilogue (B-operand fragments
  // straight from memory, as k_attn_bwd_dq loads them; rows past M read row M - 1 again and are never stored)
  constexpr int XA_WPR = XA ? 4 / (BM / 32) : 1;      // waves per 32-query block of the tile
  u4v xb_qf[XB ? 4 : 1], xb_of[XB ? 4 : 1];
  float xb_lse = 0.f;
  if constexpr (XB) {
    if (KG == 1 || kg == 0) {
      int m = m0 + (wave_s / XA_WPR) * 32 + ln;
      m = m < p.M ? m : p.M - 1;
      const T* qp = reinterpret_cast<const T*>(p.xa_q) + (size_t)m * p.xa_ldq + n0 + 8 * hi;
      const T* op = reinterpret_cast<const T*>(p.xa_o) + (size_t)m * p.xa_ldo + n0 + 8 * hi;
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        xb_qf[kk] = *reinterpret_cast<const u4v*>(qp + 16 * kk);
        xb_of[kk] = *reinterpret_cast<const u4v*>(op + 16 * kk);
      }
      const int b = div_small(m0, __builtin_amdgcn_rcpf((float)p.xa_Nq));
      xb_lse = p.xa_lse[((size_t)b * p.xa_H + blockIdx.y) * p.xa_Nq + (m - b * p.xa_Nq)] * LOG2E;
    }
  }

  constexpr int KK = BK / 16 / WG;                // k-steps of a tile multiplied by this wave group
  const int kk0 = grp * KK;
  // The K loop carries as little VALU work as it can: a wave's own vector instructions (and those of the wave it shares a
  // SIMD with) do not hide under its MFMAs (tools/ubench_coissue.hip).  The eight fragment addresses of a tile are a per-lane
  // offset per k-step (hoisted: the swizzle is an XOR, so the four k-steps are four registers) plus a wave-uniform stage
  // base kept in a scalar register and rotated without a division.
  unsigned fa_off[BK / 16], fb_off[BK / 16];
#pragma unroll
  for (int kk = 0; kk < BK / 16; ++kk) {
    const unsigned pc = (unsigned)(((2 * kk + hi) ^ ((ln >> 1) & 7)) << 4);
    fa_off[kk] = (unsigned)((wm * RPW + ln) * 128) + pc;
    fb_off[kk] = (unsigned)(BM * 128 + (wn * CPW + ln) * 128) + pc;
  }
  int stg = 0;                     // kt % ST
  DH_STAMP(2);
  for (int kt = 0; kt < loop_tiles; ++kt) {
    DH_STAMP_T(kt, 0);
    // tile kt has landed once at most (ST-2) later tiles' loads are still outstanding
    if (ntiles - 1 - kt >= ST - 2) wait_vmcnt<NP * (ST - 2)>(); else wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();
    DH_STAMP_T(kt, 1);
    if (kt == 0) DH_STAMP(3);
    if (KG > 1 && kt >= ntiles) continue;           // a group with a shorter K range only keeps the barrier count
    const bool more = ABL != 2 && kt + ST - 1 < ntiles;
    const int cur = __builtin_amdgcn_readfirstlane(stg);
    const int nkt = kt + ST - 1, nstage = cur == 0 ? ST - 1 : cur - 1;        // (kt + ST - 1) % ST
    stg = cur + 1 == ST ? 0 : cur + 1;
    if (ABL == 1) { if (more) issue(nkt, nstage); continue; }
    const unsigned char* st_base = smem + cur * STAGE;
    uint4 fw[2][TN], fx[2][TM];
    auto load_frags = [&](int kk, int buf) {
      const unsigned char* pb = st_base + fb_off[kk];
      const unsigned char* pa = st_base + fa_off[kk];
#pragma unroll
      for (int j = 0; j < TN; ++j) fw[buf][j] = *reinterpret_cast<const uint4*>(pb + j * (32 * 128));
#pragma unroll
      for (int i = 0; i < TM; ++i) fx[buf][i] = *reinterpret_cast<const uint4*>(pa + i * (32 * 128));
    };
    load_frags(kk0, 0);
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) {
      if (kk + 1 < KK) load_frags(kk0 + kk + 1, (kk + 1) & 1);      // next fragments fly under this step's MFMAs
      DH_PRIO(1);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = Mfma<T>::run(fw[kk & 1][j], fx[kk & 1][i], acc[i][j]);
      DH_PRIO(0);
      // the two waves that share a row block (wn = 0 / 1) read the same A fragments: each sums every other k-step, so the
      // v_dot2c work per wave is half and fits under the MFMAs of the step; the halves are exchanged after the loop
      if (LNF && (kk & 1) == wn_u LNF_ABL(1)) {
#pragma unroll
        for (int i = 0; i < TM; ++i) frag_sums<T>(fx[kk & 1][i], ln1[i], ln2[i]);
      }
      // the DMA of tile kt+ST-1 is issued piecewise behind the MFMAs (address VALU co-issues with the matrix pipe)
      if (more) {
        // a two-stage ring has ONE tile in flight: the moment its last piece is issued bounds the start of the next tile, so
        // the pieces go out over the first two k-steps instead of all four (128x320 conv at batch 8: 77.5 -> 71.6 us)
        constexpr int EK = ST == 2 ? 2 : KK;      // k-steps over which the pieces are spread
        if (kk < EK) {
#pragma unroll
          for (int q = kk * NP / EK; q < (kk + 1) * NP / EK; ++q) issue_piece(nkt, nstage, q);
        }
      }
    }
    if (more) next_tile();
    DH_STAMP_T(kt, 2);
  }
  DH_STAMP(4);

  if (LNF LNF_ABL(2)) {
    // exchange the row sums with the partner wave (wave ^ 1: same rows, the other k-steps) through the idle rings
    float* xb = reinterpret_cast<float*>(smem_all);
    const int wid = tid >> 6;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < TM; ++i) { xb[(wid * 2 * TM + 2 * i) * 64 + lane] = ln1[i]; xb[(wid * 2 * TM + 2 * i + 1) * 64 + lane] = ln2[i]; }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      ln1[i] += xb[((wid ^ 1) * 2 * TM + 2 * i) * 64 + lane];
      ln2[i] += xb[((wid ^ 1) * 2 * TM + 2 * i + 1) * 64 + lane];
    }
  }

  if (WG > 1 || KG > 1) {
    // add the other groups' partial sums in group order: f32 through the (now idle) rings, [value][lane] per wave
    constexpr int NG = WG * KG;
    constexpr int SLOT = (TM * TN * 16 + (LNF ? 2 * TM : 0)) * 64;
    static_assert((NG - 1) * 4 * SLOT * 4 <= KG * ST * STAGE, "merge buffer does not fit the stage rings");
    const int g = WG > 1 ? grp : kg;
    float* cb = reinterpret_cast<float*>(smem_all);
    __syncthreads();
    if (g > 0) {
      float* slot = cb + ((g - 1) * 4 + wave) * SLOT + lane;
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
          for (int r = 0; r < 16; ++r) slot[((i * TN + j) * 16 + r) * 64] = acc[i][j][r];
      if (LNF) {
#pragma unroll
        for (int i = 0; i < TM; ++i) { slot[(TM * TN * 16 + 2 * i) * 64] = ln1[i]; slot[(TM * TN * 16 + 2 * i + 1) * 64] = ln2[i]; }
      }
    }
    __syncthreads();
    if (g > 0) return;
#pragma unroll
    for (int og = 1; og < NG; ++og) {
      const float* slot = cb + ((og - 1) * 4 + wave) * SLOT + lane;
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[i][j][r] += slot[((i * TN + j) * 16 + r) * 64];
      if (LNF) {
#pragma unroll
        for (int i = 0; i < TM; ++i) { ln1[i] += slot[(TM * TN * 16 + 2 * i) * 64]; ln2[i] += slot[(TM * TN * 16 + 2 * i + 1) * 64]; }
      }
    }
  }

  if (LNF LNF_ABL(4)) {
    // row statistics: the two lanes of a row (lane, lane ^ 32) hold the halves of every k-step; then
    // acc <- rstd * (acc - mean * s[n]) + t[n], and the ordinary epilogue follows (bias is inside t)
    const float inv_k = 1.f / (float)p.K;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const float a = xor32_sum(ln1[i]), q = xor32_sum(ln2[i]);
      const float mean = a * inv_k;
      float var = q * inv_k - mean * mean;
      var = var > 0.f ? var : 0.f;
      const float rstd = rsqrtf(var + p.ln_eps);
      const int m = m0 + wm * RPW + i * 32 + ln;
      if (blockIdx.y == 0 && wn == 0 && hi == 0 && m < p.M) { p.ln_stats[2 * (size_t)m] = mean; p.ln_stats[2 * (size_t)m + 1] = rstd; }
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int n = n0 + wn * CPW + j * 32 + 8 * g + 4 * hi;
          if (n >= p.N) continue;
          float4 sv, tv;
          if (PRE_LN) { sv = lsp[PRE_LN ? j : 0][g]; tv = ltp[PRE_LN ? j : 0][g]; }
          else { sv = *reinterpret_cast<const float4*>(p.ln_s + n); tv = *reinterpret_cast<const float4*>(p.ln_t + n); }
          acc[i][j][4 * g] = rstd * (acc[i][j][4 * g] - mean * sv.x) + tv.x;
          acc[i][j][4 * g + 1] = rstd * (acc[i][j][4 * g + 1] - mean * sv.y) + tv.y;
          acc[i][j][4 * g + 2] = rstd * (acc[i][j][4 * g + 2] - mean * sv.z) + tv.z;
          acc[i][j][4 * g + 3] = rstd * (acc[i][j][4 * g + 3] - mean * sv.w) + tv.w;
        }
    }
  }

  if constexpr (XA) {
    // Cross-attention of this head.  The rounded q tile (what the unfused kernel would read back) goes to LDS at the padded row
    // stride of attention.hip, K and V behind it; then every 32-row block of the tile is one wave's queries (64-row tiles: two
    // waves per block, one half of the head dimension of O each) and the products are k_attn_fwd's -- S^T = K Q^T with the keys
    // past Nk masked, ONE exact softmax over all keys (no running maximum: they all sit in registers), O^T = V^T P^T with P
    // rounded to 16 bits -- fully unrolled over the three 32-key blocks.  The backward form (XB) stages its dO tile the same way and
    // runs k_attn_bwd_dq's products: P = exp2(S c - lse), dP^T = V dO^T, dS = P (dP - delta), dQ^T = K^T dS^T, scaled once at the end.
    typedef T T4 __attribute__((ext_vector_type(4)));
    static_assert((BM + 2 * XA_KEYS) * TLD * 2 <= KG * ST * STAGE, "q, K and V tiles fit the idle rings");
    unsigned short* sq = reinterpret_cast<unsigned short*>(smem_all);
    unsigned short* sk = sq + BM * TLD;
    unsigned short* sv = sk + XA_KEYS * TLD;
    const bool hb = p.bias != nullptr;
    __syncthreads();                                 // every wave is done with the rings / the merge buffers
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int row = wm * RPW + i * 32 + ln, m = m0 + row;
      uint2 w[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        float v0 = acc[i][0][4 * g], v1 = acc[i][0][4 * g + 1], v2 = acc[i][0][4 * g + 2], v3 = acc[i][0][4 * g + 3];
        if (hb) { const float4 b = bpre[0][g]; v0 += b.x; v1 += b.y; v2 += b.z; v3 += b.w; }
        T4 o;
        o[0] = from_f32<T>(v0); o[1] = from_f32<T>(v1); o[2] = from_f32<T>(v2); o[3] = from_f32<T>(v3);
        w[g] = __builtin_bit_cast(uint2, o);
      }
      const uint4 ca = half_exchange(w[0], w[1]), cb = half_exchange(w[2], w[3]);
      if (!XB && p.xa_save && m < p.M) {
        T* orow = reinterpret_cast<T*>(p.C) + (size_t)m * p.ldc + n0 + wn * CPW + 8 * hi;
        *reinterpret_cast<uint4*>(orow) = ca;
        *reinterpret_cast<uint4*>(orow + 16) = cb;
      }
      *reinterpret_cast<uint4*>(&sq[row * TLD + wn * CPW + 8 * hi]) = ca;
      *reinterpret_cast<uint4*>(&sq[row * TLD + wn * CPW + 8 * hi + 16]) = cb;
    }
#pragma unroll
    for (int j = 0; j < XA_CH; ++j) {
      const int idx = tid + j * 256;
      *reinterpret_cast<u4v*>(&sk[(idx >> 3) * TLD + (idx & 7) * 8]) = xa_kr[j];
      *reinterpret_cast<u4v*>(&sv[(idx >> 3) * TLD + (idx & 7) * 8]) = xa_vr[j];
    }
    __syncthreads();
    constexpr int WPR = XA_WPR, NDT = 2 / WPR;      // waves per 32-query block, 32-wide halves of the head dimension per wave
    const int rb = wave_s / WPR, dt0 = (wave_s % WPR) * NDT;
    uint4 qf[4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) qf[kk] = *reinterpret_cast<const uint4*>(&sq[(rb * 32 + ln) * TLD + 16 * kk + 8 * hi]);
    const int t16 = lane & 15;
    const int tr_off = (4 * hi + (t16 >> 2)) * TLD + 16 * ((lane >> 4) & 1) + 4 * (t16 & 3);      // (tr_frag's per-lane tile offset)
    if constexpr (XB) {
      // qf holds the dO fragments of the wave's rows; delta = rowsum(dO o O) from the fragments, as the unfused kernel sums it
      typedef T T8 __attribute__((ext_vector_type(8)));
      uint4 sqf[4];
      float del = 0.f;
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const T8 ov = __builtin_bit_cast(T8, xb_of[kk]), dv = __builtin_bit_cast(T8, qf[kk]);
#pragma unroll
        for (int c = 0; c < 8; ++c) del += to_f32<T>(ov[c]) * to_f32<T>(dv[c]);
        sqf[kk] = __builtin_bit_cast(uint4, xb_qf[kk]);
      }
      del = xor32_sum(del);
      const unsigned short* kt = sk + tr_off;
      v16f dqa[NDT];
#pragma unroll
      for (int d = 0; d < NDT; ++d) dqa[d] = zero16();
#pragma unroll
      for (int kb = 0; kb < XA_KEYS / 32; ++kb) {
        v16f sc = tile_times_frags<T>(sk, kb * 32, ln, hi, sqf);
        const v16f dp = tile_times_frags<T>(sv, kb * 32, ln, hi, qf);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float pr = kb * 32 + acc_row(r, hi) < p.xa_Nk ? fast_exp2(__builtin_fmaf(sc[r], CEXP, -xb_lse)) : 0.f;
          sc[r] = pr * (dp[r] - del);
        }
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
          const uint4 dsf = pack8<T>(sc, s2);
#pragma unroll
          for (int d = 0; d < NDT; ++d) dqa[d] = Mfma<T>::run(tr_frag(kt, (dt0 + d) * 32, kb * 32 + 16 * s2), dsf, dqa[d]);
        }
      }
      const int m = m0 + rb * 32 + ln;
      if (m < p.M) {
        T* orow = reinterpret_cast<T*>(p.xa_dq) + (size_t)m * p.xa_lddq + n0 + 8 * hi;
#pragma unroll
        for (int d = 0; d < NDT; ++d) {
          uint2 w[4];
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            T4 o;
#pragma unroll
            for (int c = 0; c < 4; ++c) o[c] = from_f32<T>(dqa[d][4 * g + c] * SCALE);
            w[g] = __builtin_bit_cast(uint2, o);
          }
          const uint4 ca = half_exchange(w[0], w[1]), cb = half_exchange(w[2], w[3]);
          *reinterpret_cast<uint4*>(orow + (dt0 + d) * 32) = ca;
          *reinterpret_cast<uint4*>(orow + (dt0 + d) * 32 + 16) = cb;
        }
      }
      return;
    }
    v16f sc[XA_KEYS / 32];
#pragma unroll
    for (int kb = 0; kb < XA_KEYS / 32; ++kb) {
      sc[kb] = tile_times_frags<T>(sk, kb * 32, ln, hi, qf);
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if (kb * 32 + acc_row(r, hi) >= p.xa_Nk) sc[kb][r] = -INFINITY;
    }
    float mx = sc[0][0];
#pragma unroll
    for (int kb = 0; kb < XA_KEYS / 32; ++kb)
#pragma unroll
      for (int r = 0; r < 16; ++r) mx = fmaxf(mx, sc[kb][r]);
    mx = xor32_max(mx);
    const float mc = mx * CEXP;
    float l = 0.f;
#pragma unroll
    for (int kb = 0; kb < XA_KEYS / 32; ++kb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        sc[kb][r] = fast_exp2(__builtin_fmaf(sc[kb][r], CEXP, -mc));
        l += sc[kb][r];
      }
    l = xor32_sum(l);
    const unsigned short* vt = sv + tr_off;
    v16f oa[NDT];
#pragma unroll
    for (int d = 0; d < NDT; ++d) oa[d] = zero16();
#pragma unroll
    for (int kb = 0; kb < XA_KEYS / 32; ++kb)
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        const uint4 pf = pack8<T>(sc[kb], s2);
#pragma unroll
        for (int d = 0; d < NDT; ++d) oa[d] = Mfma<T>::run(tr_frag(vt, (dt0 + d) * 32, kb * 32 + 16 * s2), pf, oa[d]);
      }
    const int m = m0 + rb * 32 + ln;
    if (m < p.M) {
      const float inv_l = 1.f / l;
      T* orow = reinterpret_cast<T*>(p.xa_o) + (size_t)m * p.xa_ldo + n0 + 8 * hi;
#pragma unroll
      for (int d = 0; d < NDT; ++d) {
        uint2 w[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          T4 o;
#pragma unroll
          for (int c = 0; c < 4; ++c) o[c] = from_f32<T>(oa[d][4 * g + c] * inv_l);
          w[g] = __builtin_bit_cast(uint2, o);
        }
        const uint4 ca = half_exchange(w[0], w[1]), cb = half_exchange(w[2], w[3]);
        *reinterpret_cast<uint4*>(orow + (dt0 + d) * 32) = ca;
        *reinterpret_cast<uint4*>(orow + (dt0 + d) * 32 + 16) = cb;
      }
      if (hi == 0 && dt0 == 0) {
        const int b = div_small(m0, __builtin_amdgcn_rcpf((float)p.xa_Nq));
        p.xa_lse[((size_t)b * p.xa_H + blockIdx.y) * p.xa_Nq + (m - b * p.xa_Nq)] = (mc + log2f(l)) * LN2;
      }
    }
    return;
  }

  if constexpr (GLU == 1) {
    // GEGLU forward.  Lane (ln, hi) owns value columns {8 g + 4 hi ..+3} (g = 0, 1) of every 32-column block and their gates
    // (g = 2, 3): 8 outputs per block, computed from the ROUNDED pre-activations (what the backward pass reads back), stored as
    // one 16-byte chunk per lane after the lane-pair exchange.
    typedef T T4 __attribute__((ext_vector_type(4)));
    const bool hb = p.bias != nullptr;
    T* Y = reinterpret_cast<T*>(p.glu_y);
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int m = m0 + wm * RPW + i * 32 + ln;
      if (m >= p.M) continue;
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int nb = n0 + wn * CPW + j * 32;
        if (nb >= p.N) continue;
        uint2 w[4];
        float pv[4][4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          float v0 = acc[i][j][4 * g], v1 = acc[i][j][4 * g + 1], v2 = acc[i][j][4 * g + 2], v3 = acc[i][j][4 * g + 3];
          if (hb) {
            float4 b = bpre[PRE_B ? j : 0][g];
            if (!pre_b) b = *reinterpret_cast<const float4*>(p.bias + nb + 8 * g + 4 * hi);
            v0 += b.x; v1 += b.y; v2 += b.z; v3 += b.w;
          }
          T4 o;
          o[0] = from_f32<T>(v0); o[1] = from_f32<T>(v1); o[2] = from_f32<T>(v2); o[3] = from_f32<T>(v3);
          w[g] = __builtin_bit_cast(uint2, o);
#pragma unroll
          for (int c = 0; c < 4; ++c) pv[g][c] = to_f32<T>(o[c]);
        }
        if (p.C) {
          T* out = reinterpret_cast<T*>(p.C) + (size_t)m * p.ldc + nb + 8 * hi;
          *reinterpret_cast<uint4*>(out) = half_exchange(w[0], w[1]);
          *reinterpret_cast<uint4*>(out + 16) = half_exchange(w[2], w[3]);
        }
        uint2 y[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          T4 o;
#pragma unroll
          for (int c = 0; c < 4; ++c) o[c] = from_f32<T>(pv[q][c] * gelu_f(pv[q + 2][c]));
          y[q] = __builtin_bit_cast(uint2, o);
        }
        *reinterpret_cast<uint4*>(Y + (size_t)m * p.glu_ldy + (nb >> 1) + 8 * hi) = half_exchange(y[0], y[1]);
      }
    }
    return;
  }
  // GEGLU backward.  The tile holds dy (natural output columns o); the saved pre-activations of output columns
  // [o0, o0 + 32) are the two paired 32-column blocks at 2 o0 + 32 q.  Per block the lane pair loads the value / gate chunks
  // (16 bytes each), un-exchanges them to the (g, hi) ownership of the accumulators, and stores d_value / d_gate as
  // 16-byte chunks after the inverse exchange.  Every load is issued before the first use.
  // Column-split form (p.glub_f < N: a transformer's proj_out folded into ff.net.2): only the tiles left of the seam hold dy of
  // the GEGLU; the others fall through to the plain epilogue below (their C / R are passed shifted by glub_f columns).
  if (GLU == 2 && glub_tile_is_glu(n0, p.glub_f)) {
    typedef T T4 __attribute__((ext_vector_type(4)));
    const T* X = reinterpret_cast<const T*>(p.glub_x);
    T* DX = reinterpret_cast<T*>(p.glub_dx);
    const size_t ldx = 2 * (size_t)p.glub_f;
    uint4 Hc[TM][TN][2], Gc[TM][TN][2];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int m = m0 + wm * RPW + i * 32 + ln;
      const int mc = m < p.M ? m : p.M - 1;
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        int nb = n0 + wn * CPW + j * 32;
        if (nb >= p.glub_f) nb = 0;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const T* src = X + (size_t)mc * ldx + 2 * nb + 32 * q + 8 * hi;
          Hc[i][j][q] = *reinterpret_cast<const uint4*>(src);
          Gc[i][j][q] = *reinterpret_cast<const uint4*>(src + 16);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int m = m0 + wm * RPW + i * 32 + ln;
      if (m >= p.M) continue;
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int nb = n0 + wn * CPW + j * 32;
        if (nb >= p.glub_f) continue;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const uint4 hc = Hc[i][j][q], gc = Gc[i][j][q];
          const uint4 hx = half_exchange(make_uint2(hc.x, hc.y), make_uint2(hc.z, hc.w));
          const uint4 gx = half_exchange(make_uint2(gc.x, gc.y), make_uint2(gc.z, gc.w));
          uint2 dh[2], dg[2];
#pragma unroll
          for (int s2 = 0; s2 < 2; ++s2) {
            const int g = 2 * q + s2;
            const T4 hh = __builtin_bit_cast(T4, s2 ? make_uint2(hx.z, hx.w) : make_uint2(hx.x, hx.y));
            const T4 gg = __builtin_bit_cast(T4, s2 ? make_uint2(gx.z, gx.w) : make_uint2(gx.x, gx.y));
            T4 oh, og;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
              const float dy = acc[i][j][4 * g + c], gate = to_f32<T>(gg[c]);
              const GeluParts gp = gelu_parts(gate);
              oh[c] = from_f32<T>(dy * gate * gp.Phi);
              og[c] = from_f32<T>(dy * to_f32<T>(hh[c]) * fmaf(gate, gp.pdf, gp.Phi));
            }
            dh[s2] = __builtin_bit_cast(uint2, oh);
            dg[s2] = __builtin_bit_cast(uint2, og);
          }
          T* dst = DX + (size_t)m * ldx + 2 * nb + 32 * q + 8 * hi;
          *reinterpret_cast<uint4*>(dst) = half_exchange(dh[0], dh[1]);
          *reinterpret_cast<uint4*>(dst + 16) = half_exchange(dg[0], dg[1]);
        }
      }
    }
    return;
  }
  DH_STAMP(5);
  // GroupNorm statistics of the output in THIS kernel's epilogue (p.gn_epi, round 6): the next op normalises the tensor being
  // written, and where K is not split there is no reduce kernel to carry the slice statistics, so a k_gn_partial launch re-read
  // the tensor just to sum it.  The rounded outputs are still in registers here: per lane column sums over its TM rows, a
  // half-wave reduction over the 32 rows of a block (DPP), the wave rows and the columns of a group through LDS in a fixed
  // order, and the tile leaves (n, mean, M2) of every group fragment it covers as "slice" 2 * row_tile + part of the
  // [b][g][3][S] layout k_gn_apply merges (part 1 = the tail of a group whose first channel lies in the previous column tile;
  // a group wholly inside the tile writes an empty part 1).
  // The forward sums are pivot-shifted: every column of a wave is summed relative to its value in the wave's first row (lane 0 /
  // lane 32 of row block 0: broadcast by readlane for that row block, kept for the others in a per-wave table at the start of the
  // idle rings -- 32 more registers per lane would spill the 256x128 tile), so a group mean of many standard deviations, carried
  // by the bias or by the inputs alike, does not cancel digits in sum(x^2) - sum(x)^2 / n; the (wave, column) pieces are merged
  // as (mean, M2) pairs (Chan) in gn_finish.
  constexpr bool GNE = gn_epi_fwd_tile(BN, GLU, LNF);
  const bool gn_epi = GNE && p.splits == 1 && (p.gn_epi == 1 || (GNB && p.gn_epi == 2));     // (the dispatch asks for form 2 only on GNB tiles)
  static_assert(!GNE || NWV * CPW * 4 <= KG * ST * STAGE - 4096, "the pivot table lies below the column-sum scratch");
  float* gpt = reinterpret_cast<float*>(smem_all) + wave * CPW;      // this wave's column pivots
  if (GNE && gn_epi && !(GNB && gnb)) __syncthreads();             // every wave is done with the rings / the merge buffers
  float gsa[GNE ? TN : 1][16], gsq[GNE ? TN : 1][16];
  if (GNE) {
#pragma unroll
    for (int j = 0; j < (GNE ? TN : 1); ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) { gsa[j][r] = 0.f; gsq[j][r] = 0.f; }
  }
  auto gn_acc = [&](int i, int j, int g, uint2 packed) {
    if constexpr (GNE) {
      typedef T T4g __attribute__((ext_vector_type(4)));
      const T4g ov = __builtin_bit_cast(T4g, packed);
      float v[4], pv[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) v[c] = to_f32<T>(ov[c]);
      float4* pt = reinterpret_cast<float4*>(gpt + j * 32 + 8 * g + 4 * hi);
      if (i == 0) {        // (every row of the tile is valid when the dispatch asks for the statistics: the wave is whole here)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int p0 = __builtin_amdgcn_readlane(__float_as_int(v[c]), 0), p1 = __builtin_amdgcn_readlane(__float_as_int(v[c]), 32);
          pv[c] = __int_as_float(hi ? p1 : p0);
        }
        if (ln == 0) *pt = make_float4(v[0], v[1], v[2], v[3]);
      } else {
        const float4 t = *pt;
        pv[0] = t.x; pv[1] = t.y; pv[2] = t.z; pv[3] = t.w;
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) { const float d = v[c] - pv[c]; gsa[j][4 * g + c] += d; gsq[j][4 * g + c] += d * d; }
    }
  };
  // BACKWARD flavour (gnb): the tile is dy of the GroupNorm (+ SiLU) whose input tile sits in rpre; the per-element terms are
  // k_gn_partial<bwd>'s -- d = dy * gamma * act'(xhat gamma + beta), the sums of d and d * xhat -- and the slices carry the plain
  // sums ([b][g][S][2], what k_gn_bwd_apply adds up).  The per-column constants come from a 64-entry table in LDS.
  const float4* gnb_tab = reinterpret_cast<const float4*>(smem_all + KG * ST * STAGE - 2048) + wn * CPW + 4 * hi;
  if constexpr (GNB) {
    if (gnb) {
      float4* tab = reinterpret_cast<float4*>(smem_all + KG * ST * STAGE - 2048);
      __syncthreads();                               // every wave is done with the rings / the merge buffers
      if (tid < BN) tab[tid] = gnb_col;
      __syncthreads();
    }
  }
  // (the four table entries of a chunk are read where they are used, once per row block: all sixteen of a lane held across the
  //  epilogue were 64 more registers, which took the 74-KB 128x64 tile from two workgroups per CU to one)
  auto gnb_acc = [&](int g, uint2 packed, uint2 xraw) {
    if constexpr (GNB) {
      typedef T T4g __attribute__((ext_vector_type(4)));
      const T4g ov = __builtin_bit_cast(T4g, packed), xv = __builtin_bit_cast(T4g, xraw);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float4 t = gnb_tab[8 * g + c];
        const float xh = (to_f32<T>(xv[c]) - t.z) * t.w;
        float d = to_f32<T>(ov[c]);
        if (p.gnb_silu) d *= silu_grad(xh * t.x + t.y);
        d *= t.x;
        gsa[0][4 * g + c] += d; gsq[0][4 * g + c] += d * xh;
      }
    }
  };
  auto gn_finish = [&]() {
    if constexpr (GNE) {
      constexpr int CS_BYTES = WMS * BN * 2 * 4;
      static_assert(CS_BYTES <= (GNB ? 2048 : 4096) && KG * ST * STAGE >= 8192, "column-sum scratch lives in the last 4 KiB of the ring (the backward table in its upper half)");
      float* cs = reinterpret_cast<float*>(smem_all + KG * ST * STAGE - 4096);
      __syncthreads();                               // every wave is done with the rings / the merge buffers
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float a = gsa[j][r], q = gsq[j][r];
          a = oct_sum(a); q = oct_sum(q);
          a += dpp_f32<DPP_ROW_MIRROR>(a); q += dpp_f32<DPP_ROW_MIRROR>(q);
          { const LanePair pa = row_pair(a); a = pa.a + pa.b; }
          { const LanePair pq = row_pair(q); q = pq.a + pq.b; }
          if (ln == 0) {
            const int col = wn * CPW + j * 32 + 8 * (r >> 2) + 4 * hi + (r & 3);
            // forward: (mean, M2) of the column's RPW rows in this wave; backward: the plain sums
            const float2 v2 = (GNB && gnb) ? make_float2(a, q) : make_float2(gpt[j * 32 + 8 * (r >> 2) + 4 * hi + (r & 3)] + a * (1.f / RPW),
                                                                             q - a * a * (1.f / RPW));
            *reinterpret_cast<float2*>(cs + (wm * BN + col) * 2) = v2;
          }
        }
      __syncthreads();
      const int cpg = p.gn_cpg, G = p.gn_G, Sx = p.gn_S;
      const int f = tid >> 3, sub = tid & 7;
      const int g = n0 / cpg + f;
      if (tid < (BN / 8) * 8 && g < G && g * cpg < n0 + BN) {
        const int lo = g * cpg, hi_c = lo + cpg;
        const int c_lo = (lo > n0 ? lo : n0) - n0, c_hi = (hi_c < n0 + BN ? hi_c : n0 + BN) - n0;
        const int b = m0 / p.gn_HW, rt = (m0 - b * p.gn_HW) / BM;
        const int part = lo < n0 ? 1 : 0;
        if (GNB && gnb) {
          float a = 0.f, q = 0.f;
          for (int c = c_lo + sub; c < c_hi; c += 8) {
#pragma unroll
            for (int w2 = 0; w2 < WMS; ++w2) { const float2 v = *reinterpret_cast<const float2*>(cs + (w2 * BN + c) * 2); a += v.x; q += v.y; }
          }
          a = oct_sum(a); q = oct_sum(q);
          if (sub == 0) {
            float2* o = reinterpret_cast<float2*>(p.gn_part) + (size_t)(b * G + g) * Sx + 2 * rt + part;
            o[0] = make_float2(a, q);
            if (part == 0 && hi_c <= n0 + BN) o[1] = make_float2(0.f, 0.f);
          }
        } else {
          // Chan over the WMS x (c_hi - c_lo) column pieces of RPW rows each: the mean relative to the first piece, then
          // M2 = sum M2_c + RPW sum (mean_c - mean)^2
          const float ref = cs[c_lo * 2];
          float dm = 0.f;
          for (int c = c_lo + sub; c < c_hi; c += 8) {
#pragma unroll
            for (int w2 = 0; w2 < WMS; ++w2) dm += cs[(w2 * BN + c) * 2] - ref;
          }
          dm = oct_sum(dm);
          const float pieces = (float)WMS * (float)(c_hi - c_lo);
          const float mean = ref + dm / pieces;
          float m2 = 0.f;
          for (int c = c_lo + sub; c < c_hi; c += 8) {
#pragma unroll
            for (int w2 = 0; w2 < WMS; ++w2) {
              const float2 v = *reinterpret_cast<const float2*>(cs + (w2 * BN + c) * 2);
              const float d = v.x - mean;
              m2 += v.y + (float)RPW * d * d;
            }
          }
          m2 = oct_sum(m2);
          if (sub == 0) {
            float* o = p.gn_part + ((size_t)(b * G + g) * 3) * Sx + 2 * rt + part;
            o[0] = (float)RPW * pieces; o[Sx] = mean; o[2 * Sx] = m2;
            if (part == 0 && hi_c <= n0 + BN) { o[1] = 0.f; o[Sx + 1] = 0.f; o[2 * Sx + 1] = 0.f; }      // the whole group lies in this tile
          }
        }
      }
    }
  };
  // the common epilogue as straight-line code: bias and residual already sit in registers (prefetched under the K loop), no
  // per-image vector, no SiLU.  The general path below carries a fallback load and a ~90-instruction SiLU block per 4-column
  // group behind uniform branches; jumping over them costs an instruction-cache line fetch per hop in a kernel whose
  // epilogue runs once, on one wave per SIMD.
  if (PRE && p.splits == 1 && p.wide_store && p.pre_r && !p.rowvec && !p.act_silu LEAN_ABL) {
    typedef T T4 __attribute__((ext_vector_type(4)));
    const bool hb = p.bias != nullptr, hr = p.R != nullptr;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int m = m0 + wm * RPW + i * 32 + ln;
      if (m >= p.M) continue;
      T* orow = reinterpret_cast<T*>(p.C) + (size_t)m * p.ldc + n0 + wn * CPW + 8 * hi;
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        if (n0 + wn * CPW + j * 32 >= p.N) continue;
        uint2 w[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          float v0 = acc[i][j][4 * g], v1 = acc[i][j][4 * g + 1], v2 = acc[i][j][4 * g + 2], v3 = acc[i][j][4 * g + 3];
          if (hb) {
            float4 b = bpre[PRE_B ? j : 0][g];
            if (!PRE_B) b = *reinterpret_cast<const float4*>(p.bias + n0 + wn * CPW + j * 32 + 8 * g + 4 * hi);
            v0 += b.x; v1 += b.y; v2 += b.z; v3 += b.w;
          }
          if (hr) {
            const T4 rv = __builtin_bit_cast(T4, rpre[i][j][g]);
            v0 += to_f32<T>(rv[0]); v1 += to_f32<T>(rv[1]); v2 += to_f32<T>(rv[2]); v3 += to_f32<T>(rv[3]);
          }
          T4 o;
          o[0] = from_f32<T>(v0); o[1] = from_f32<T>(v1); o[2] = from_f32<T>(v2); o[3] = from_f32<T>(v3);
          w[g] = __builtin_bit_cast(uint2, o);
          if (gn_epi) { if (GNB && gnb) gnb_acc(g, w[g], rpre[i][j][g]); else gn_acc(i, j, g, w[g]); }
        }
        const uint4 ca = half_exchange(w[0], w[1]), cb = half_exchange(w[2], w[3]);
        *reinterpret_cast<uint4*>(orow + j * 32) = ca;
        *reinterpret_cast<uint4*>(orow + j * 32 + 16) = cb;
      }
      if (GNB && gnb) asm volatile("" ::: "memory");      // the next row block re-reads its table entries
    }
    if (gn_epi) gn_finish();
    DH_STAMP(6);
#ifdef DH_TUNING
    if (p.ts) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); DH_STAMP(7); }
#endif
    return;
  }
  // 16-bit results: the two lanes of a row (lane, lane ^ 32) own alternating 4-column groups; they swap two groups so
  // that each stores two 16-byte chunks instead of four 8-byte ones (half the write transactions, whole 32-byte sectors
  // per lane pair)
  if (p.splits == 1 && p.wide_store) {
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int m = m0 + wm * RPW + i * 32 + ln;
      if (m >= p.M) continue;                       // both lanes of a pair share m
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int nb = n0 + wn * CPW + j * 32;
        if (nb >= p.N) continue;                    // N is a multiple of 32 on this path
        uint2 w[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          w[g] = epilogue_pack<T>(p, m, nb + 8 * g + 4 * hi, acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2],
                                  acc[i][j][4 * g + 3], pre_r, rpre[i][j][g], pre_b, bpre[PRE_B ? j : 0][g]);
          if (gn_epi) gn_acc(i, j, g, w[g]);
        }
        const uint4 ca = half_exchange(w[0], w[1]), cb = half_exchange(w[2], w[3]);
        T* out = reinterpret_cast<T*>(p.C) + (size_t)m * p.ldc + nb + 8 * hi;
        *reinterpret_cast<uint4*>(out) = ca;
        *reinterpret_cast<uint4*>(out + 16) = cb;
      }
    }
    if (gn_epi) gn_finish();
    DH_STAMP(6);
#ifdef DH_TUNING
    if (p.ts) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); DH_STAMP(7); }
#endif
    return;
  }

#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int m = m0 + wm * RPW + i * 32 + ln;
    if (m >= p.M) continue;
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int n = n0 + wn * CPW + j * 32 + 8 * g + 4 * hi;
        if (n >= p.N) continue;
        if (p.splits > 1) {
          float4 o = make_float4(acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]);
          *reinterpret_cast<float4*>(p.partial + ((size_t)blockIdx.z * p.M + m) * p.N + n) = o;
        } else {
          epilogue_store<T>(p, m, n, acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3], pre_r,
                            rpre[i][j][g], pre_b, bpre[PRE_B ? j : 0][g]);
        }
      }
  }
}

// plain [N][K] (K contiguous) -> tiled layout, for the test hooks (the engine tiles at load time)
template <class T>
__global__ void k_tile_weights(const T* src, T* dst, int N, int K, int conv_cin) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)N * K) return;
  const int n = (int)(idx / K);
  int k = (int)(idx - (size_t)n * K);
  if (conv_cin) { const int tap = k / conv_cin; k = conv_k_index(tap, k - tap * conv_cin); }
  dst[wt_index(n, k, K)] = src[idx];
}
void launch_tile_weights(int dtype, const void* src, void* dst, int N, int K, hipStream_t st, int conv_cin) {
  const unsigned nb = (unsigned)(((size_t)N * K + 255) / 256);
  hipLaunchKernelGGL((k_tile_weights<unsigned short>), dim3(nb), dim3(256), 0, st, (const unsigned short*)src, (unsigned short*)dst, N, K, conv_cin);
}

template <class T>
__global__ void k_splitk_reduce(const GemmK p) {
  const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;   // index of a 4-wide group
  const size_t total = (size_t)p.M * p.N / 4;
  if (q >= total) return;
  const size_t e = q * 4;
  const int m = (int)((unsigned)e / (unsigned)p.N), n = (int)((unsigned)e - (unsigned)m * (unsigned)p.N);     // M * N < 2^32
  // every load of the element group is issued before the first add: bias / residual first, slabs four at a time
  const bool have_r = p.R != nullptr, have_b = p.bias != nullptr;
  const uint2 rpre = have_r ? *reinterpret_cast<const uint2*>(reinterpret_cast<const T*>(p.R) + (size_t)m * p.ldr + n) : make_uint2(0, 0);
  const float4 bpre = have_b ? *reinterpret_cast<const float4*>(p.bias + n) : make_float4(0.f, 0.f, 0.f, 0.f);
  const size_t slab = (size_t)p.M * p.N;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  int z = 0;
  for (; z + 4 <= p.splits; z += 4) {
    float4 v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = *reinterpret_cast<const float4*>(p.partial + (size_t)(z + j) * slab + e);
#pragma unroll
    for (int j = 0; j < 4; ++j) { s.x += v[j].x; s.y += v[j].y; s.z += v[j].z; s.w += v[j].w; }
  }
  for (; z < p.splits; ++z) {
    const float4 v = *reinterpret_cast<const float4*>(p.partial + (size_t)z * slab + e);
    s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
  }
  epilogue_store<T>(p, m, n, s.x, s.y, s.z, s.w, have_r, rpre, have_b, bpre);
}

// split-K reduce fused with the GroupNorm slice statistics of its output (the next op of a resnet's conv is a
// GroupNorm): workgroup = (row slice, 4 groups, image) like k_gn_partial; a thread sums the slabs of 8 channels of a
// row, applies the epilogue, stores the 16-bit result and accumulates the pivot-shifted sums of the ROUNDED values.
template <class T, bool BWD>
__global__ void __launch_bounds__(256) k_splitk_reduce_gn(const GemmK p) {
  __shared__ float sm_red[4][2 * GN_GB];
  __shared__ float sm_piv[GN_GB];
  const int HW = p.gn_HW, G = p.gn_G, S = p.gn_S;
  const int s = blockIdx.x, g0 = blockIdx.y * GN_GB, b = blockIdx.z, cpg = div_small(p.N, rcp_fast(G));
  const int W = GN_GB * cpg, nch = W >> 3;
  const float inv_nch = rcp_fast(nch), inv_S = rcp_fast(S), inv_cpg = rcp_fast(cpg);
  const int RP = div_small((int)blockDim.x, inv_nch);
  const int r0 = div_small(HW * s, inv_S), r1 = div_small(HW * (s + 1), inv_S);
  const size_t slab = (size_t)p.M * p.N;
  // forward sums are pivot-shifted like k_gn_partial's, by the group's first element of the slice (row r0): the threads of
  // row r0 publish it through LDS after their first row, so a group mean of many standard deviations (from the bias or from
  // the inputs) does not cancel digits in sum(x^2) - sum(x)^2 / n; slices are merged with Chan's formula in the apply kernel
  const int rr = div_small((int)threadIdx.x, inv_nch), ch = threadIdx.x - rr * nch;
  float ga[GN_GB], gq[GN_GB];
#pragma unroll
  for (int gl = 0; gl < GN_GB; ++gl) { ga[gl] = 0.f; gq[gl] = 0.f; }
  const int n = g0 * cpg + ch * 8;
  const bool live = rr < RP && n < p.N;
  int gi[8];
  float av[8], qv[8], pv[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    gi[i] = div_small(ch * 8 + i, inv_cpg);
    av[i] = 0.f; qv[i] = 0.f; pv[i] = 0.f;
  }
  float bias8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float gm[8], bt[8], mu[8], rs[8];
  if (live) {
    if (p.bias) {
      *reinterpret_cast<float4*>(bias8) = *reinterpret_cast<const float4*>(p.bias + n);
      *reinterpret_cast<float4*>(bias8 + 4) = *reinterpret_cast<const float4*>(p.bias + n + 4);
    }
    if (BWD) {           // output = dy of a GroupNorm: accumulate sum d and sum d * xhat (d = dy * gamma * act')
      *reinterpret_cast<float4*>(gm) = *reinterpret_cast<const float4*>(p.gnb_gamma + n);
      *reinterpret_cast<float4*>(gm + 4) = *reinterpret_cast<const float4*>(p.gnb_gamma + n + 4);
      *reinterpret_cast<float4*>(bt) = *reinterpret_cast<const float4*>(p.gnb_beta + n);
      *reinterpret_cast<float4*>(bt + 4) = *reinterpret_cast<const float4*>(p.gnb_beta + n + 4);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int sg = b * G + g0 + gi[i];
        mu[i] = p.gnb_stats[2 * sg]; rs[i] = p.gnb_stats[2 * sg + 1];
      }
    }
  }
  // one row of the thread's 8 channels: reduce the slabs, apply the epilogue, store the 16-bit result; the forward returns the
  // rounded values in f, the backward accumulates its sums
  auto row = [&](int r, float* f) {
    const int m = b * HW + r;
    float v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = 0.f;
    const float* pp = p.partial + (size_t)m * p.N + n;
    int z = 0;
    for (; z + 4 <= p.splits; z += 4) {             // four slabs in flight; added in slab order
      float4 x0[4], x1[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        x0[j] = *reinterpret_cast<const float4*>(pp + (size_t)(z + j) * slab);
        x1[j] = *reinterpret_cast<const float4*>(pp + (size_t)(z + j) * slab + 4);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        v[0] += x0[j].x; v[1] += x0[j].y; v[2] += x0[j].z; v[3] += x0[j].w;
        v[4] += x1[j].x; v[5] += x1[j].y; v[6] += x1[j].z; v[7] += x1[j].w;
      }
    }
    for (; z < p.splits; ++z) {
      const float4 x0 = *reinterpret_cast<const float4*>(pp + (size_t)z * slab);
      const float4 x1 = *reinterpret_cast<const float4*>(pp + (size_t)z * slab + 4);
      v[0] += x0.x; v[1] += x0.y; v[2] += x0.z; v[3] += x0.w;
      v[4] += x1.x; v[5] += x1.y; v[6] += x1.z; v[7] += x1.w;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] += bias8[i];
    if (p.rowvec) {
      const float* rv = p.rowvec + (size_t)div_small(m, p.inv_rows_per_batch) * p.rowvec_ld + n;
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] += rv[i];
    }
    if (p.act_silu) {
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = v[i] / (1.f + __expf(-v[i]));
    }
    if (p.R) {
      const uint4 raw = *reinterpret_cast<const uint4*>(reinterpret_cast<const T*>(p.R) + (size_t)m * p.ldr + n);
      const T* rv = reinterpret_cast<const T*>(&raw);
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] += to_f32<T>(rv[i]);
    }
    T o[8];
    if (!BWD) {
#pragma unroll
      for (int i = 0; i < 8; ++i) { o[i] = from_f32<T>(v[i]); f[i] = to_f32<T>(o[i]); }
    } else {
      const uint4 rawx = *reinterpret_cast<const uint4*>(reinterpret_cast<const T*>(p.gnb_x) + (size_t)m * p.gnb_ldx + n);
      const T* xv = reinterpret_cast<const T*>(&rawx);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        o[i] = from_f32<T>(v[i]);
        const float xh = (to_f32<T>(xv[i]) - mu[i]) * rs[i];
        float d = to_f32<T>(o[i]);
        if (p.gnb_silu) d *= silu_grad(xh * gm[i] + bt[i]);
        d *= gm[i];
        av[i] += d; qv[i] += d * xh;
      }
    }
    *reinterpret_cast<uint4*>(reinterpret_cast<T*>(p.C) + (size_t)m * p.ldc + n) = *reinterpret_cast<uint4*>(o);
  };
  auto acc = [&](const float* f) {
#pragma unroll
    for (int i = 0; i < 8; ++i) { const float d = f[i] - pv[i]; av[i] += d; qv[i] += d * d; }
  };
  float f[8];
  if (BWD) {
    if (live)
      for (int r = r0 + rr; r < r1; r += RP) row(r, f);
  } else {
    // the first row of every thread, then the pivots: row r0 of each group's first channel (a slice has >= 4 rows)
    const bool first = live && r0 + rr < r1;
    if (first) row(r0 + rr, f);
    if (first && rr == 0) {
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if (ch * 8 + i == gi[i] * cpg) sm_piv[gi[i]] = f[i];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 8; ++i) pv[i] = g0 + gi[i] < G ? sm_piv[gi[i]] : 0.f;
    if (first) {
      acc(f);
      for (int r = r0 + rr + RP; r < r1; r += RP) { row(r, f); acc(f); }
    }
  }
  if (live) {
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int gl = 0; gl < GN_GB; ++gl) {
        ga[gl] += gi[i] == gl ? av[i] : 0.f;
        gq[gl] += gi[i] == gl ? qv[i] : 0.f;
      }
  }
#pragma unroll
  for (int gl = 0; gl < GN_GB; ++gl) { ga[gl] = wave_sum(ga[gl]); gq[gl] = wave_sum(gq[gl]); }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int gl = 0; gl < GN_GB; ++gl) { sm_red[threadIdx.x >> 6][2 * gl] = ga[gl]; sm_red[threadIdx.x >> 6][2 * gl + 1] = gq[gl]; }
  }
  __syncthreads();
  if ((int)threadIdx.x < GN_GB && g0 + (int)threadIdx.x < G) {
    const int gl = threadIdx.x, g = g0 + gl;
    float sa = 0.f, sq = 0.f;
    for (int w = 0; w < 4; ++w) { sa += sm_red[w][2 * gl]; sq += sm_red[w][2 * gl + 1]; }
    if (BWD) {
      p.gn_part[((size_t)(b * G + g) * S + s) * 2] = sa;
      p.gn_part[((size_t)(b * G + g) * S + s) * 2 + 1] = sq;
    } else {
      const float cnt = (float)(r1 - r0) * (float)cpg;
      float* o = p.gn_part + ((size_t)(b * G + g) * 3) * S + s;
      o[0] = cnt; o[S] = sm_piv[gl] + sa / cnt; o[2 * S] = sq - sa * sa / cnt;
    }
  }
}

// one tile configuration, the A-operand mode and the folded-LayerNorm variant picked at run time
// (profiled launches carry their own start / stop events: the elapsed time between them is the kernel's execution time as
// the command processor stamps it, the figure rocprofv3 --kernel-trace reports, not a bracket that contains the dispatch)
#define DH_GEMM_LAUNCH(KERNEL)                                                                              \
  do {                                                                                                      \
    if (g_prof.e0) hipExtLaunchKernelGGL(KERNEL, grid, dim3(TH), 0, st, g_prof.e0, g_prof.e1, 0, k);        \
    else hipLaunchKernelGGL(KERNEL, grid, dim3(TH), 0, st, k);                                              \
  } while (0)
template <class T, int BM, int BN, int ST, int WG, int KG, int MW, bool BUF>
static void launch_tile_b(int gm, bool lnf, dim3 grid, hipStream_t st, const GemmK& k, int glu) {
  constexpr int TH = 256 * WG * KG * MW;
  // the tiles that carry the GEGLU epilogues (pick_tile picks only these when glu != 0)
  constexpr bool GLUOK = WG == 1 && KG == 1 && ((BM == 256 && BN == 128 && MW == 2) || (BM == 128 && BN == 128 && MW == 2 && ST == 4) || (BM == 64 && BN == 64));
  if constexpr (GLUOK) {
    if (glu == 1 && lnf) { DH_GEMM_LAUNCH((k_gemm_dma<T, BM, BN, ST, GM_DENSE, 0, WG, KG, MW, true, 1, BUF>)); return; }
    if (glu == 1) { DH_GEMM_LAUNCH((k_gemm_dma<T, BM, BN, ST, GM_DENSE, 0, WG, KG, MW, false, 1, BUF>)); return; }
    if (glu == 2) { DH_GEMM_LAUNCH((k_gemm_dma<T, BM, BN, ST, GM_DENSE, 0, WG, KG, MW, false, 2, BUF>)); return; }
  }
  if constexpr (xattn_epi_tile(BM, BN, WG, MW, BUF)) {
    if (glu == EPI_XATTN && lnf) { DH_GEMM_LAUNCH((k_gemm_dma<T, BM, BN, ST, GM_DENSE, 0, WG, KG, MW, true, EPI_XATTN, BUF>)); return; }
    if (glu == EPI_XATTN) { DH_GEMM_LAUNCH((k_gemm_dma<T, BM, BN, ST, GM_DENSE, 0, WG, KG, MW, false, EPI_XATTN, BUF>)); return; }
    if (glu == EPI_XATTN_DQ) { DH_GEMM_LAUNCH((k_gemm_dma<T, BM, BN, ST, GM_DENSE, 0, WG, KG, MW, false, EPI_XATTN_DQ, BUF>)); return; }
  }
  if (gm == GM_DENSE) {
    if constexpr (WG == 1 && BN != 320 && BN != 160) {      // (the 128x320 / 128x160 tiles are never asked for the folded LayerNorm)
      if (lnf) { DH_GEMM_LAUNCH((k_gemm_dma<T, BM, BN, ST, GM_DENSE, 0, WG, KG, MW, true, 0, BUF>)); return; }
    }
    DH_GEMM_LAUNCH((k_gemm_dma<T, BM, BN, ST, GM_DENSE, 0, WG, KG, MW, false, 0, BUF>));
  } else if (gm == GM_CONV_S1) {
    DH_GEMM_LAUNCH((k_gemm_dma<T, BM, BN, ST, GM_CONV_S1, 0, WG, KG, MW, false, 0, BUF>));
  } else {
    DH_GEMM_LAUNCH((k_gemm_dma<T, BM, BN, ST, GM_GENERIC, 0, WG, KG, MW>));
  }
}
// k.pp_a_bytes != 0: the operands fit buffer descriptors (plan_extents) -- dense and stride-1 3x3 launches stage through them
template <class T, int BM, int BN, int ST, int WG, int KG, int MW>
static void launch_tile(int gm, bool lnf, dim3 grid, hipStream_t st, const GemmK& k, int glu = 0) {
  g_launched_tile = LaunchedTile{BM, BN, KG, ST, MW};
  if (k.pp_a_bytes != 0 && gm != GM_GENERIC) launch_tile_b<T, BM, BN, ST, WG, KG, MW, true>(gm, lnf, grid, st, k, glu);
  else launch_tile_b<T, BM, BN, ST, WG, KG, MW, false>(gm, lnf, grid, st, k, glu);
}
#undef DH_GEMM_LAUNCH

// ---- the plan: what one launch will be, decided on the host without touching the device (gemm_k.h: GemmPlan) --------------------------
// Tile / split-K policy.  The constants are the round-1/2 bench.py A/B winners; a tuning build (-DDH_TUNING,
// tools/lab.sh build-tuning) reads them from the environment instead, the product library carries no knobs.
#ifdef DH_TUNING
#define DH_KNOB(name, env, dflt) static const int name = getenv(env) ? atoi(getenv(env)) : (dflt)
#else
#define DH_KNOB(name, env, dflt) constexpr int name = (dflt)
#endif
DH_KNOB(kSplitTiles, "DH_SPLITK_TILES", 200);     // split K only under this many output tiles ...
DH_KNOB(kSplitMinK, "DH_SPLITK_MINKT", 32);       // ... and from this many K tiles (24 -> 32: +1 % on the guided step)
DH_KNOB(kSplitTarget, "DH_SPLITK_TARGET", 256);   // workgroups aimed at
DH_KNOB(kBigTiles, "DH_BIG_TILES", 128);          // fewer big tiles than this and a short K loop: 64x64 tiles (48 -> 128: +1 % step, +2 % at 768^2)
DH_KNOB(kNarrowTiles, "DH_NARROW_TILES", 40);     // long-K GEMMs with at most this many 128x128 tiles use the 128x64 tile
DH_KNOB(kN320, "DH_GEMM_N320", 224);              // row tiles from which N = 320 runs as one 128x320 tile (256 at batch 8: pass -4.5 %; 144 tiles lose 1 %)
DH_KNOB(kMwBlocks, "DH_GEMM_MW", 64);             // 256x128 eight-wave tiles from this many of them
DH_KNOB(kMwShortK, "DH_GEMM_MW_SHORTK", 128);     // ... from this many of them when the K loop is short (pick_tile)
DH_KNOB(kT160, "DH_GEMM_T160", 224);              // fewest 128x160 tiles for that tile (0 = never)
DH_KNOB(kKg2MinKt, "DH_KG2_MINKT", 4);            // K tiles per split from which the 128x64 tile splits K over two wave groups (16 -> 4: +1.4 % step)
DH_KNOB(kManyBlocks, "DH_GEMM_MANY", 512);        // 128x128 grids from this size use two stages (two workgroups per CU)
DH_KNOB(kMw128, "DH_GEMM_MW128", 1);              // min K tiles for eight waves on the 128x128 tile
DH_KNOB(kTwoPerCu, "DH_GEMM_TWO_PER_CU", 1);      // 128x64 grids of 257..512 workgroups: the 74-KB three-stage tile, two workgroups per CU (pick_instance)
#undef DH_KNOB

static int glu_form(const GemmK& k) { return k.glu_y ? 1 : (k.glub_x ? 2 : 0); }
static int gemm_mode(const GemmK& k) {
  if (k.mode == A_DENSE) return GM_DENSE;
  return (k.mode == A_CONV3 && k.stride == 1 && k.up == 0 && k.pad == 1) ? GM_CONV_S1 : GM_GENERIC;
}

// Step 1, the k_gemm_dma tile.  The three flags say which rule set it: later rules and the cross-attention form ask for them.
struct TilePick { int bm, bn; bool n320, mw2, t160; };
static TilePick pick_tile(const GemmK& k, int glu, bool lnf) {
  TilePick t{128, (k.N % 128 == 0) ? 128 : 64, false, false, false};
  const int ktiles = k.K / BK;
  if (t.bn == 128 && ktiles >= 16 && cdiv(k.M, 128) * cdiv(k.N, 128) <= kNarrowTiles) t.bn = 64;
  // few output tiles and a K loop too short to be worth slabs + a reduce launch: 64x64 tiles
  // (M=256 N=1280 K=1280: 16.7 -> 8.8 us; M=1024 N=640 K=640: 12.1 -> 8.9 us)
  if (k.M <= 64 || (cdiv(k.M, 128) * cdiv(k.N, t.bn) < kBigTiles && ktiles < kSplitMinK)) { t.bm = 64; t.bn = 64; }
  // N = 320 (the 64x64-latent convolutions and linears) with enough rows to fill the chip: one 128x320 tile per 128 rows,
  // so the A tile is staged once instead of five times (batched edits; a single image has only 32 such tiles)
  // (also N = 640 / 960 -- the fused q|k|v projection of the 64x64-latent level -- as two / three such column tiles: the A tile is
  //  staged three times instead of fifteen)
  t.n320 = kN320 > 0 && k.N % 320 == 0 && k.N <= 960 && !lnf && t.bm == 128 && t.bn == 64 && cdiv(k.M, 128) >= kN320;
  if (t.n320) t.bn = 320;
  // grids that fill the machine: 256x128 tiles, eight waves (see MW)
  // (not when M <= 256 leaves a single row of 256-row tiles on fewer than half of the CUs: two rows of 128x128 eight-wave
  // tiles put twice the workgroups on the same K loop -- M = 256, N = 10240, K = 1280: 22.4 -> 15.5 us)
  // and in general not for short K loops on fewer than half of the CUs (per-shape sweep, tools/sweep_gemm_shapes.py:
  // M = 1024, N = 2560, K = 640: 16.6 -> 12.8 us; M = 512, N = 5120, K = 1280: 25.2 -> 20.2 us as 128x128 tiles); long K
  // loops keep the big tile, they split K over workgroups anyway
  const long tiles256 = (long)cdiv(k.M, 256) * cdiv(k.N, 128);
  t.mw2 = kMwBlocks > 0 && k.N % 128 == 0 && tiles256 >= kMwBlocks &&
          !(k.M <= 256 && k.M > 128 && cdiv(k.N, 128) < 128) && (tiles256 >= kMwShortK || ktiles >= kSplitMinK);
  // (tried and dropped, profiles/r04_ab_two128.txt: a 256x128 grid of 129..255 workgroups -- M = 8192, N = 640 at batch 8: 160 -- as twice
  //  as many 128x128 two-stage tiles, two per CU: conv K = 5760 91.6 -> 95.9 us, batch-8 forward 12.74 -> 13.05 ms; the smaller tile
  //  stages a third more bytes per flop and that outweighs the 96 CUs it wakes up)
  if (t.mw2) { t.bm = 256; t.bn = 128; }
  // GEGLU epilogues (dense, N a multiple of 128 -- of 64 for the column-split backward -- never split): 64x64, 128x128 or 256x128
  // tiles only
  if (glu && !(t.bm == 64 && t.bn == 64)) { t.bm = t.mw2 ? 256 : 128; t.bn = 128; }
  // the column-split GEGLU backward: no tile straddles the seam (the last column tile may run past N: W is readable there)
  if (glu == 2 && !glub_split_ok(t.bn, k.glub_f)) { t.bm = 64; t.bn = 64; t.mw2 = false; }
  // 128x160 tiles (four wave rows of 32 x 160) where exactly they fill the chip in ONE round and nothing needs K split: the
  // batched 32x32-latent level (M = 8192, N = 640: 64 x 4 = 256 workgroups instead of 160 256x128 ones) and its kin
  const long tiles160 = (long)cdiv(k.M, 128) * (k.N / 160);
  t.t160 = kT160 > 0 && k.N % 160 == 0 && !lnf && !glu && !t.n320 && t.bm != 64 && tiles160 >= kT160 && tiles160 <= 256;
  if (t.t160) { t.bm = 128; t.bn = 160; }
  return t;
}

// Step 2, the K split of a k_gemm_dma launch (k_gemm_pp brings its own: gemm_pp_plan)
static int pick_splits(const GemmK& k, size_t partial_elems, int tiles, int glu, bool lnf) {
  const int ktiles = k.K / BK;
  if (!(k.partial && !lnf && !glu && tiles < kSplitTiles && ktiles >= kSplitMinK)) return 1;
  return clamp_splits(kSplitTarget / tiles, ktiles / 4, 32, k, partial_elems);
}

// steps 1 and 2 together: the kernel family, its tile, the K split asked for (plan_finish cuts K evenly and may end with fewer)
struct PlanDraft { bool pp; TilePick t; int splits; };
static PlanDraft plan_draft(const GemmK& k, size_t partial_elems, const GemmHooks& h) {
  const int glu = glu_form(k);
  const bool lnf = k.ln_s != nullptr;
  PlanDraft d;
  // grids that fill the chip with 256- / 128-row tiles and carry the plain epilogue: the eight-wave ping-pong kernel (gemm_pp.hip)
  PpPlan pp;
  d.pp = gemm_pp_plan(k, partial_elems, h, &pp);
  d.t = pick_tile(k, glu, lnf);
  if (d.pp) { d.t.bm = pp.bm; d.t.bn = pp.bn; d.splits = pp.splits; }
  else d.splits = pick_splits(k, partial_elems, cdiv(k.M, d.t.bm) * cdiv(k.N, d.t.bn), glu, lnf);
  return d;
}

// Step 3, the descriptor extents: buffer-descriptor staging (BUF instantiations) whenever both operands lie below 2 GiB and the rows
// are 16-byte aligned (every launch of the U-Net / VAE / text engines; anything else keeps the address form).  k_gemm_pp always
// stages through descriptors (gemm_pp_plan has checked the same bounds).
static void plan_extents(GemmPlan& p, const GemmK& k, const GemmHooks& h) {
  const size_t ab = gemm_a_bytes(k);
  if (p.pp) { p.a_bytes = (unsigned)ab; p.w_bytes = (unsigned)((size_t)k.N * k.K * 2); p.buf = 1; return; }
  const size_t wb = (size_t)align_up((size_t)k.N, 64) * k.K * 2;
  const bool conv_ok = k.mode == A_DENSE || (k.Cin % 64 == 0 && k.K == 9 * k.Cin);
  if ((h.buf_stage & 1) && ab > 0 && conv_ok && ab + (size_t)(k.Win + 1) * k.lda * 2 < 0x7ff00000ull && wb < 0x7ff00000ull && k.lda % 8 == 0 &&
      ((size_t)k.A & 15) == 0 && ((size_t)k.W & 15) == 0) {
    p.a_bytes = (unsigned)ab; p.w_bytes = (unsigned)wb;
  }
  p.buf = p.a_bytes != 0 && p.gm != GM_GENERIC;
}

// Step 4, what rides along in the epilogue of an unsplit k_gemm_dma launch.  Each form is one predicate here, one GemmPlan field
// and one arm of launch_tile_b.  (The GEGLU forms are not optional: glu_form() is part of the request and pick_tile gives them a
// tile that carries them.)
// GroupNorm statistics, either direction: tiles of whole images' rows, groups no wider than a column tile, at most 64 "slices" = 2 per
// row tile for the merge in k_gn_apply.  *gn_done then carries the slice count (> 1) instead of 1.
static bool gn_epi_shape_ok(const GemmK& k, const GemmPlan& p) {
  if (!(p.splits == 1 && !p.pp && k.gn_part && k.gn_G > 0 && k.gn_HW > 0 && k.C && k.wide_store && k.M % k.gn_HW == 0 &&
        k.gn_HW % p.bm == 0 && k.N % k.gn_G == 0 && k.N % p.bn == 0)) return false;
  const int cpg = k.N / k.gn_G, sx = 2 * (k.gn_HW / p.bm);
  return cpg >= 8 && cpg <= p.bn && sx <= 64;
}
// forward statistics: the next op normalises this launch's output
static bool gn_epi_fwd_ok(const GemmK& k, const GemmPlan& p, const GemmHooks& h, int glu) {
  return (h.buf_stage & 4) == 0 && gn_epi_fwd_tile(p.bn, glu, p.lnf) && !k.gnb_x && h.gn_done && gn_epi_shape_ok(k, p);
}
// ... and the BACKWARD slice statistics (sum d, sum d * xhat) when the output is dy of a GroupNorm: 64-column tiles of up to 128
// rows, no bias / residual / per-image vector (an input-gradient GEMM has none; the residual's prefetch registers carry the
// GroupNorm's input tile)
static bool gn_epi_bwd_ok(const GemmK& k, const GemmPlan& p, const GemmHooks& h, int glu) {
  return (h.buf_stage & 8) == 0 && gn_epi_bwd_tile(p.bm, p.bn, 1, glu, p.lnf) && k.gnb_x && h.gn_done && gn_epi_shape_ok(k, p) && k.pre_r &&
         !k.R && !k.bias && !k.rowvec && !k.act_silu && (((size_t)k.gnb_x | (size_t)(k.gnb_ldx * 2)) & 7) == 0;
}
// Cross-attention (EPI_XATTN): the q projection of a cross-attention whose 64-column tiles are whole heads and whose row tiles lie
// inside one image (a tile never mixes two images' K / V), unsplit, with the plain bias-only epilogue, at most XA_KEYS keys, every
// operand 16-byte aligned; its dQ (EPI_XATTN_DQ) in the to_out input-gradient GEMM, with no bias and no folded LayerNorm.
// *xa_done tells the caller that the attention has been launched with the GEMM.
static bool xattn_epi_ok(const GemmK& k, const GemmPlan& p, const TilePick& t, const GemmHooks& h, int glu) {
  const bool bwd = k.xa_dq != nullptr;
  return k.xa_o && h.xa_done && (h.buf_stage & (bwd ? 32 : 16)) == 0 && p.splits == 1 && !p.pp && !glu && !t.t160 && !t.n320 && !t.mw2 &&
         xattn_epi_tile(p.bm, p.bn, 1, 1, p.a_bytes != 0) && p.gm == GM_DENSE && k.xa_Nk >= 1 && k.xa_Nk <= XA_KEYS && k.xa_Nq > 0 &&
         k.N == 64 * k.xa_H && k.M % k.xa_Nq == 0 && k.M < (1 << 22) && (k.M == k.xa_Nq || k.xa_Nq % p.bm == 0) && k.C && k.wide_store && k.pre_r &&
         !k.R && !k.rowvec && !k.act_silu && !p.gn_epi && k.xa_lse && k.xa_ldk % 8 == 0 && k.xa_ldo % 8 == 0 &&
         (((size_t)k.xa_k | (size_t)k.xa_v | (size_t)k.xa_o) & 15) == 0 &&
         (!bwd || (!p.lnf && !k.bias && k.xa_q && k.xa_ldq % 8 == 0 && k.xa_lddq % 8 == 0 && (((size_t)k.xa_q | (size_t)k.xa_dq) & 15) == 0));
}

// Step 5, the instantiation of the tile: ring stages, K groups, wave multiplier (the arms of launch_planned's switch)
static void pick_instance(GemmPlan& p, int glu, int tiles_per_split) {
  const long wgs = (long)p.grid[0] * p.grid[1] * p.splits;
  auto set = [&](int st, int kg, int mw) { p.stages = st; p.wg = 1; p.kg = kg; p.mw = mw; };
  if (p.bn == 160) set(4, 1, 1);
  else if (p.bm == 256) set(3, 1, 2);
  else if (p.bm == 128 && p.bn == 128 && (glu || (kMw128 && tiles_per_split >= kMw128))) set(4, 1, 2);
  // between one and two workgroups per CU (the 96x96-latent level of a 768x768 image: 72 x 5 = 360 tiles; the B = 2 CFG pass at
  // 64x64 latents: 64 x 5 = 320): the 147-KB two-group tile fits one workgroup per CU, so such a grid runs as two rounds with the
  // second one mostly empty; a three-stage ring without the K groups is 74 KB, two workgroups share a CU and the grid is one round
  // (same-box A/B, profiles/r04_ab_two_per_cu.txt: B = 2 forward 5.46 -> 5.30 ms, backward 6.82 -> 6.67 ms; 96x96 latents bf16 B = 1
  // forward 6.49 -> 6.32 ms, backward 9.55 -> 9.40 ms; guided step 34.97 -> 35.30 steps/s)
  else if (kTwoPerCu && p.bm == 128 && p.bn == 64 && wgs > 256 && wgs <= 512) set(3, 1, 1);
  // two wave groups on disjoint K ranges: measured ahead only on the 128x64 tile (conv 4096x320x2880: 28.5 -> 24.9 us,
  // x5760: 50.8 -> 42.7 us; 128x128 tiles and short loops lose to the merge; 64x64 tiles: no K grouping wins in situ)
  else if (p.bm == 128 && p.bn == 64 && tiles_per_split >= kKg2MinKt) set(3, 2, 1);
  // eight waves (4 x 2, 32 x 160 outputs each): the two-stage ring has one 57-KB tile in flight and its 56 one-KiB DMA pieces were
  // issued by four waves, 14 each at 60 - 185 cycles apiece -- the issue, not the latency, bounded the tile; with seven pieces per
  // wave: M = 32768, N = 320 dense K = 320 20.6 -> 14.9 us, K = 1280 40.1 -> 34.6 us, conv K = 2880 76.8 -> 67.3 us, batch-8
  // forward 13.55 -> 13.15 ms (profiles/r04_ab_n320_eight_waves.txt)
  else if (p.bn == 320) set(2, 1, 2);
  else if (p.bm == 64) set(4, 1, 1);      // (rings of 6 / 8 stages: pass 2 % SLOWER; round 3, eight stages only on the <= 256-workgroup long-K launches: guided step -1.1 %)
  else if (p.bn == 128 && kManyBlocks > 0 && wgs >= kManyBlocks) set(2, 1, 1);   // 64 KiB: two workgroups per CU
  else if (p.bn == 128) set(4, 1, 1);
  else set(5, 1, 1);
}

// Step 6, the launch after a split GEMM: the plain reduce, or one that also leaves the GroupNorm slice statistics of the summed output
// (forward, or backward when it is dy of a GroupNorm), or -- the rows are the dy of a LayerNorm -- reduce + LayerNorm backward in one
// launch (dy itself is not written)
static int pick_reduce(const GemmK& k, const GemmPlan& p, const GemmHooks& h) {
  if (p.splits <= 1) return RED_NONE;
  if (k.gn_part && k.gn_G > 0 && k.gn_HW > 0 && k.N % k.gn_G == 0 && (GN_GB * (k.N / k.gn_G)) % 8 == 0 &&
      GN_GB * (k.N / k.gn_G) <= 2048 && k.M % k.gn_HW == 0) return k.gnb_x ? RED_GN_BWD : RED_GN_FWD;
  if (k.lnb_x && h.lnb_done && !k.bias && !k.rowvec && !k.R && !k.act_silu && k.N % 8 == 0 && k.ldc == k.N) return RED_LN_BWD;
  return RED_PLAIN;
}

// the cut (K tiles spread evenly over the splits) and steps 3 - 6
static GemmPlan plan_finish(const PlanDraft& d, const GemmK& k, const GemmHooks& h) {
  GemmPlan p{};
  const int glu = glu_form(k), ktiles = k.K / BK;
  p.pp = d.pp ? 1 : 0; p.bm = d.t.bm; p.bn = d.t.bn; p.lnf = k.ln_s != nullptr; p.gm = gemm_mode(k);
  const int tiles_per_split = cdiv(ktiles, d.splits);
  p.splits = cdiv(ktiles, tiles_per_split);
  p.k_per_split = tiles_per_split * BK;
  if (gn_epi_fwd_ok(k, p, h, glu)) p.gn_epi = 1;
  if (gn_epi_bwd_ok(k, p, h, glu)) p.gn_epi = 2;
  if (p.gn_epi) { p.gn_cpg = k.N / k.gn_G; p.gn_S = 2 * (k.gn_HW / p.bm); }
  plan_extents(p, k, h);
  if (xattn_epi_ok(k, p, d.t, h, glu)) p.xa = k.xa_dq ? 2 : 1;
  p.epi = p.xa == 2 ? EPI_XATTN_DQ : (p.xa ? EPI_XATTN : glu);
  if (p.pp) {
    // persistent grid: one workgroup per CU (256: a multiple of 8, the XCD order of the work items holds in every round)
    const unsigned nwork = (unsigned)(cdiv(k.M, p.bm) * (k.N / p.bn) * p.splits);
    p.grid[0] = (h.pp_persist == 0 || nwork <= (unsigned)h.cus) ? nwork : (unsigned)h.cus; p.grid[1] = p.grid[2] = 1;
  } else {
    p.grid[0] = cdiv(k.M, p.bm); p.grid[1] = cdiv(k.N, p.bn); p.grid[2] = p.splits;
    pick_instance(p, glu, tiles_per_split);
  }
  p.reduce = pick_reduce(k, p, h);
  if (p.reduce == RED_GN_FWD || p.reduce == RED_GN_BWD) p.gn_S = gn_slices(k.gn_HW, k.M / k.gn_HW);
  return p;
}

GemmPlan gemm_plan(const GemmK& k, size_t partial_elems, const GemmHooks& h) { return plan_finish(plan_draft(k, partial_elems, h), k, h); }

// ---- the tuning build (tools/lab.sh build-tuning): everything it adds to the decision, applied to the finished plan --------------
#ifdef DH_TUNING
// per-shape policy search (tools/sweep_gemm_shapes.py): DH_GEMM_LOG=1 prints every dispatch, DH_FORCE_TILE / DH_FORCE_SPLITS override
// the choice (1 = 64x64, 2 = 128x64 two K groups, 3 = 128x64, 4 = 128x128 eight waves, 5 = 128x128, 6 = 256x128 eight waves, 7 = 128x160);
// a forced plan is the draft with the tile / split replaced, finished again, without the cross-attention form
static void tune_plan(GemmPlan& p, GemmK& k, size_t partial_elems, const GemmHooks& h) {
  static const int kLog = getenv("DH_GEMM_LOG") ? atoi(getenv("DH_GEMM_LOG")) : 0;
  static const int kWnt = getenv("DH_W_NT") ? atoi(getenv("DH_W_NT")) : 0;                     // non-temporal weight DMA for GEMMs of at most this many row tiles (0 = never)
  static const int kLnfAbl = getenv("DH_LNF_ABL") ? atoi(getenv("DH_LNF_ABL")) : 0;
  const int kForceTile = getenv("DH_FORCE_TILE") ? atoi(getenv("DH_FORCE_TILE")) : 0;          // (re-read per dispatch: one process sweeps)
  const int kForceSplits = getenv("DH_FORCE_SPLITS") ? atoi(getenv("DH_FORCE_SPLITS")) : 0;
  const bool lnf = k.ln_s != nullptr;
  PlanDraft d = plan_draft(k, partial_elems, h);
  int force_tile = 0;
  if (kForceTile && !d.pp && !glu_form(k)) {
    const int fbm = kForceTile == 1 ? 64 : (kForceTile == 6 ? 256 : 128), fbn = kForceTile == 7 ? 160 : ((kForceTile <= 3) ? 64 : 128);
    if ((k.N % fbn == 0 || fbn == 64) && !(fbn == 160 && lnf)) { d.t.bm = fbm; d.t.bn = fbn; force_tile = kForceTile; }
  }
  const bool force_splits = kForceSplits && !d.pp && k.partial && !lnf;
  if (force_splits) d.splits = clamp_splits(kForceSplits, (k.K / BK) / 2, 1 << 30, k, partial_elems);
  if (kLog) fprintf(stderr, "GEMMLOG M=%d N=%d K=%d mode=%d lnf=%d gn=%d gnb=%d bias=%d R=%d rowvec=%d | pp=%d BM=%d BN=%d splits=%d\n", k.M, k.N, k.K,
                    k.mode == A_DENSE ? 0 : (k.mode == A_CONV3 && k.stride == 1 && k.up == 0 ? 1 : 2), (int)lnf, k.gn_part != nullptr,
                    k.gnb_x != nullptr, k.bias != nullptr, k.R != nullptr, k.rowvec != nullptr, (int)d.pp, d.t.bm, d.t.bn, d.splits);
  if (force_tile || force_splits) p = plan_finish(d, k, h);
  if (force_tile) {
    static const int inst[8][3] = {{0, 0, 0}, {4, 1, 1}, {3, 2, 1}, {5, 1, 1}, {4, 1, 2}, {4, 1, 1}, {3, 1, 2}, {4, 1, 1}};      // stages, K groups, wave multiplier
    p.stages = inst[force_tile][0]; p.kg = inst[force_tile][1]; p.mw = inst[force_tile][2];
    p.xa = 0; p.epi = 0;
  }
  // DH_GEMM_LOG=2: the whole request and plan of every launch -- the rows tests/test_gemm_plan.py pins (its query fields, then
  // dh_dbg_gemm_plan's output order)
  if (kLog > 1) {
    const int conv = k.mode == A_DENSE ? 0 : (k.mode == A_CONV3 ? 1 : 2);
    const unsigned flags = (k.bias ? 1u : 0u) | (k.R ? 2u : 0u) | (k.rowvec ? 4u : 0u) | (k.act_silu ? 8u : 0u) | (lnf ? 16u : 0u) |
                           (k.gn_part ? 32u : 0u) | (k.gnb_x ? 64u : 0u) | (k.lnb_x ? 128u : 0u) | (k.glu_y ? 256u : 0u) | (k.glub_x ? 512u : 0u) |
                           (k.xa_o && !k.xa_dq ? 1024u : 0u) | (k.xa_dq ? 2048u : 0u) | ((((size_t)k.A | (size_t)k.W | (size_t)k.C) & 15) == 0 ? 4096u : 0u);
    int v[GEMM_PLAN_FIELDS];
    memcpy(v, &p, sizeof(v));
    fprintf(stderr, "GEMMPLAN q %d %d %d %d %d %d %d %ld %ld %zu %u %d %d %d %d %d %d |", k.M, k.N, k.K, conv, k.Hin, k.stride, k.up, k.lda, k.ldc,
            partial_elems, flags, k.gn_HW, k.gn_G, k.glub_x ? k.glub_f : 0, k.xa_Nq, k.xa_Nk, k.xa_H);
    for (int i = 0; i < GEMM_PLAN_FIELDS; ++i) fprintf(stderr, " %d", v[i]);
    fprintf(stderr, "\n");
  }
  k.w_nt = kWnt > 0 && cdiv(k.M, p.bm) <= kWnt;
  k.lnf_abl = kLnfAbl;
  k.ts = g_gemm_ts;
}
#else
static inline void tune_plan(GemmPlan&, GemmK&, size_t, const GemmHooks&) {}
#endif

// ---- accounting, launch, publish -------------------------------------------------------------------------------------------------------
// profiled runs (dh_gemm_profile_begin): the event pair that brackets the launch, its flops and algorithmic bytes
static void prof_account(const GemmK& k, const GemmPlan& p) {
  if (!g_prof.on) return;
  if (g_prof.used + 2 > g_prof.ev.size()) {
    const size_t old = g_prof.ev.size();
    g_prof.ev.resize(old + 4096);
    for (size_t i = old; i < g_prof.ev.size(); ++i) (void)hipEventCreate(&g_prof.ev[i]);
  }
  g_prof.e0 = g_prof.ev[g_prof.used++];
  g_prof.e1 = g_prof.ev[g_prof.used++];
  g_prof.flops += 2.0 * (double)k.M * (double)k.N * (double)k.K;
  // every operand once, in its storage type: the A source (dense rows; for a convolution the source image, not its im2col
  // view), the weights, the output (the GEGLU forms: what they read and write instead), the residual
  const double esz = 2.0;
  double a_elems = (double)k.M * k.K;
  if (k.mode != A_DENSE && k.Hout > 0 && k.Wout > 0) a_elems = (double)k.M / ((double)k.Hout * k.Wout) * k.Hin * k.Win * k.Cin;
  double c_elems = (double)k.M * k.N * (k.C ? 1.0 : 0.0) + (k.R ? (double)k.M * k.N : 0.0);
  if (k.glu_y) c_elems += 0.5 * (double)k.M * k.N;
  // saved pre-activations read [M][2F], their gradient written [M][2F] (C holds only the columns past F)
  if (k.glub_x) c_elems += 4.0 * (double)k.M * k.glub_f - (k.C ? (double)k.M * k.glub_f : 0.0);
  if (p.gn_epi == 2) c_elems += (double)k.M * k.N;       // the GroupNorm input tile the backward statistics read
  if (p.xa == 1) c_elems += (k.xa_save ? 1.0 : 0.0) * (double)k.M * k.N + 2.0 * (k.M / k.xa_Nq) * (double)k.xa_Nk * k.N;   // o for q (q too when saved), the heads' K and V
  if (p.xa == 2) c_elems += 2.0 * (double)k.M * k.N + 2.0 * (k.M / k.xa_Nq) * (double)k.xa_Nk * k.N;     // dq for dO; q, o, K and V read
  g_prof.bytes += esz * (a_elems + (double)k.N * k.K + c_elems);
}

constexpr unsigned tile_key(int bm, int bn, int st, int kg, int mw) { return (unsigned)(bm | bn << 10 | st << 20 | kg << 24 | mw << 26); }

// the plan into the argument block, the kernel the plan names, the reduce it names
template <class T>
static void launch_planned(const GemmPlan& p, GemmK k, hipStream_t st) {
  constexpr int dtype = std::is_same<T, f16>::value ? DH_DTYPE_F16 : DH_DTYPE_BF16;
  k.splits = p.splits; k.k_per_split = p.k_per_split;
  k.gn_epi = p.gn_epi; k.gn_cpg = p.gn_cpg; k.xa = p.xa;
  if (p.gn_epi) k.gn_S = p.gn_S;
  if (!p.pp) { k.pp_a_bytes = p.a_bytes; k.pp_w_bytes = p.w_bytes; }
  const dim3 grid(p.grid[0], p.grid[1], p.grid[2]);
  g_launched_tile = LaunchedTile{};
  bool ablated = false;
#ifdef DH_TUNING
  // ablations of the K loop (timing only): 1 = no LDS reads / MFMA, 2 = no DMA in the loop, 3 = 1 on the dense kernel
  static const int kAbl = getenv("DH_GEMM_ABLATE") ? atoi(getenv("DH_GEMM_ABLATE")) : 0;
  const bool t128 = !p.pp && p.bm == 128 && p.bn == 128, t256 = !p.pp && p.bm == 256;
  ablated = true;
  if (kAbl == 1 && t128) hipLaunchKernelGGL((k_gemm_dma<T, 128, 128, 4, GM_CONV_S1, 1>), grid, dim3(256), 0, st, k);
  else if (kAbl == 2 && t128) hipLaunchKernelGGL((k_gemm_dma<T, 128, 128, 4, GM_CONV_S1, 2>), grid, dim3(256), 0, st, k);
  else if (kAbl == 3 && t128) hipLaunchKernelGGL((k_gemm_dma<T, 128, 128, 4, GM_DENSE, 1>), grid, dim3(256), 0, st, k);
  else if (kAbl == 1 && t256 && p.gm == GM_CONV_S1) hipLaunchKernelGGL((k_gemm_dma<T, 256, 128, 3, GM_CONV_S1, 1, 1, 1, 2>), grid, dim3(512), 0, st, k);
  else if (kAbl == 2 && t256 && p.gm == GM_CONV_S1) hipLaunchKernelGGL((k_gemm_dma<T, 256, 128, 3, GM_CONV_S1, 2, 1, 1, 2>), grid, dim3(512), 0, st, k);
  else if (kAbl == 1 && t256 && p.gm == GM_DENSE && !p.lnf) hipLaunchKernelGGL((k_gemm_dma<T, 256, 128, 3, GM_DENSE, 1, 1, 1, 2>), grid, dim3(512), 0, st, k);
  else if (kAbl == 2 && t256 && p.gm == GM_DENSE && !p.lnf) hipLaunchKernelGGL((k_gemm_dma<T, 256, 128, 3, GM_DENSE, 2, 1, 1, 2>), grid, dim3(512), 0, st, k);
  else ablated = false;
#endif
#define DH_TILE(BM, BN, ST, KG, MW) \
  case tile_key(BM, BN, ST, KG, MW): launch_tile<T, BM, BN, ST, 1, KG, MW>(p.gm, p.lnf != 0, grid, st, k, p.epi); break
  if (ablated) {        // (tuning build: a timing ablation stood in for the planned kernel)
  } else if (p.pp) {
    PpPlan pp;
    pp.bm = p.bm; pp.bn = p.bn; pp.splits = p.splits; pp.grid = p.grid[0];
    g_launched_tile.bm = pp.bm; g_launched_tile.bn = pp.bn;
    launch_gemm_pp(dtype, k, pp, st, g_prof.e0, g_prof.e1);
  } else switch (tile_key(p.bm, p.bn, p.stages, p.kg, p.mw)) {
    DH_TILE(128, 160, 4, 1, 1);
    DH_TILE(256, 128, 3, 1, 2);
    DH_TILE(128, 128, 4, 1, 2);
    DH_TILE(128, 64, 3, 1, 1);
    DH_TILE(128, 64, 3, 2, 1);
    DH_TILE(128, 320, 2, 1, 2);
    DH_TILE(64, 64, 4, 1, 1);
    DH_TILE(128, 128, 2, 1, 1);
    DH_TILE(128, 128, 4, 1, 1);
    DH_TILE(128, 64, 5, 1, 1);
    default:               // pick_instance (or a forced tile) named a tile that is not instantiated: no kernel ran, the output is stale
      fprintf(stderr, "launch_planned: no k_gemm_dma instantiation for tile %dx%d stages %d kg %d mw %d\n", p.bm, p.bn, p.stages, p.kg, p.mw);
      abort();
  }
#undef DH_TILE
  g_prof.e0 = g_prof.e1 = nullptr;
  if (p.reduce == RED_GN_FWD || p.reduce == RED_GN_BWD) {
    k.gn_S = p.gn_S;
    const dim3 rgrid(k.gn_S, cdiv(k.gn_G, GN_GB), k.M / k.gn_HW);
    if (p.reduce == RED_GN_BWD) hipLaunchKernelGGL((k_splitk_reduce_gn<T, true>), rgrid, dim3(256), 0, st, k);
    else hipLaunchKernelGGL((k_splitk_reduce_gn<T, false>), rgrid, dim3(256), 0, st, k);
  } else if (p.reduce == RED_LN_BWD) {
    launch_splitk_reduce_ln_bwd(dtype, k.partial, p.splits, k.lnb_x, k.lnb_gamma, k.lnb_stats, k.lnb_add, k.lnb_dx, k.M, k.N, st, k.lnb_ldx);
  } else if (p.reduce == RED_PLAIN) {
    const size_t groups = (size_t)k.M * k.N / 4;
    hipLaunchKernelGGL((k_splitk_reduce<T>), dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, st, k);
  }
}

// GemmArgs -> the kernel-side argument block, every decision still open (splits = 1, no epilogue riders)
static GemmK fill_gemm_k(const GemmArgs& a) {
  GemmK k;
  k.A = a.A; k.lda = a.lda; k.W = a.W; k.M = a.M; k.N = a.N; k.K = a.K;
  k.mode = a.mode; k.Hin = a.Hin; k.Win = a.Win; k.Cin = a.Cin; k.Hout = a.Hout; k.Wout = a.Wout;
  k.stride = a.stride; k.up = a.up; k.pad = a.pad;
  k.bias = a.bias; k.rowvec = a.rowvec; k.rowvec_ld = a.rowvec_ld;
  k.rows_per_batch = a.rows_per_batch > 0 ? a.rows_per_batch : 1;
  k.inv_rows_per_batch = 1.f / (float)k.rows_per_batch;
  k.R = a.R; k.ldr = a.ldr; k.C = a.C; k.ldc = a.ldc; k.act_silu = a.act_silu;
  k.partial = a.partial; k.splits = 1; k.k_per_split = a.K;
  k.pre_r = 1;
  k.wide_store = a.N % 32 == 0 && a.ldc % 8 == 0 && ((size_t)a.C & 15) == 0;
  k.ln_s = a.ln_s; k.ln_t = a.ln_t; k.ln_stats = a.ln_stats; k.ln_eps = a.ln_eps;
  k.gn_part = a.gn_part; k.gn_HW = a.gn_HW; k.gn_G = a.gn_G; k.gn_S = 0; k.gn_epi = 0; k.gn_cpg = 0;
  k.gnb_x = a.gnb_x; k.gnb_ldx = a.gnb_ldx; k.gnb_gamma = a.gnb_gamma; k.gnb_beta = a.gnb_beta; k.gnb_stats = a.gnb_stats;
  k.gnb_silu = a.gnb_silu;
  k.lnb_x = a.lnb_x; k.lnb_ldx = a.lnb_ldx > 0 ? a.lnb_ldx : a.N;
  k.lnb_gamma = a.lnb_gamma; k.lnb_stats = a.lnb_stats; k.lnb_add = a.lnb_add; k.lnb_dx = a.lnb_dx;
  k.glu_y = a.glu_y; k.glu_ldy = a.glu_ldy; k.glub_x = a.glub_x; k.glub_dx = a.glub_dx;
  k.glub_f = a.glub_x && a.glub_f > 0 && a.glub_f < a.N ? a.glub_f : a.N;
  if (k.glub_f < a.N) {
    // the plain column block [glub_f, N) lands at column n - glub_f of C (and of R): the kernel indexes them by n
    if (k.C) k.C = reinterpret_cast<unsigned short*>(k.C) - k.glub_f;
    if (k.R) k.R = reinterpret_cast<const unsigned short*>(k.R) - k.glub_f;
  } else if (a.glub_x) {
    k.C = nullptr;        // (the whole tile is dy of the GEGLU: C is not written)
  }
  k.xa = 0; k.xa_k = a.xa_k; k.xa_v = a.xa_v; k.xa_ldk = a.xa_ldk; k.xa_o = a.xa_o; k.xa_ldo = a.xa_ldo; k.xa_lse = a.xa_lse;
  k.xa_H = a.xa_H; k.xa_Nq = a.xa_Nq; k.xa_Nk = a.xa_Nk; k.xa_save = a.xa_save;
  k.xa_q = a.xa_q; k.xa_ldq = a.xa_ldq; k.xa_dq = a.xa_dq; k.xa_lddq = a.xa_lddq;
  return k;
}

// the test hooks and the device, read once per launch
static GemmHooks current_hooks() {
  GemmHooks h;
  gemm_pp_hooks(&h);
  h.pp_force = g_pp_force; h.buf_stage = g_buf_stage;
  return h;
}

// fill, plan, account, launch, publish
double launch_gemm(int dtype, const GemmArgs& a, hipStream_t st) {
  GemmK k = fill_gemm_k(a);
  GemmHooks h = current_hooks();
  h.gn_done = a.gn_done != nullptr; h.lnb_done = a.lnb_done != nullptr; h.xa_done = a.xa_done != nullptr;
  GemmPlan p = gemm_plan(k, a.partial_elems, h);
  tune_plan(p, k, a.partial_elems, h);
  prof_account(k, p);
  if (dtype == DH_DTYPE_F16) launch_planned<f16>(p, k, st);
  else launch_planned<bf16>(p, k, st);
  // what the launch carried, for the caller (the slice count of an epilogue's GroupNorm statistics, 1 for the reduce's) and for
  // the test hooks (dh_dbg_gemm_last_tile, dh_dbg_gemm_xattn_carried)
  g_last_plan = p;
  const bool reduce_gn = p.reduce == RED_GN_FWD || p.reduce == RED_GN_BWD;
  if (a.gn_done) *a.gn_done = p.gn_epi ? p.gn_S : (reduce_gn ? 1 : 0);
  if (a.lnb_done) *a.lnb_done = p.reduce == RED_LN_BWD ? 1 : 0;
  if (a.xa_done) *a.xa_done = p.xa ? 1 : 0;
  if (p.xa) ++g_xattn_total;
  return 2.0 * (double)a.M * (double)a.N * (double)a.K;
}

}  // namespace dh

#ifdef DH_TUNING
// tuning builds: the next GEMM launches stamp the timeline of their first workgroup into `ts` (8 x u64, device memory)
extern "C" int dh_dbg_gemm_timeline(unsigned long long* ts) { dh::g_gemm_ts = ts; return DH_OK; }
#endif

// test hook: which main-loop family the next launches use (0 = the shipped policy, 1 = k_gemm_dma only, 2 = k_gemm_pp for every
// launch it can carry) -- parity tests run small shapes through both, tools/bench_gemm_pp.py times them side by side
extern "C" int dh_dbg_gemm_family(int force) {
  DH_REQUIRE(force >= 0 && force <= 2, "family: 0 policy, 1 k_gemm_dma, 2 k_gemm_pp");
  dh::g_pp_force = force;
  return DH_OK;
}

// test hook: 1 = dense / stride-1 3x3 operands of k_gemm_dma stage through buffer descriptors (shipped), 0 = through addresses
extern "C" int dh_dbg_gemm_stage(int buf) {
  dh::g_buf_stage = buf;          // bit 0: buffer staging; bit 2 (value 4): NO GroupNorm forward statistics in the GEMM epilogue; bit 3 (8): NO backward ones; bit 4 (16): NO cross-attention in the q projection's epilogue; bit 5 (32): NO cross-attention dQ in the to_out input-gradient's epilogue
  return DH_OK;
}

// test hook: the tile the last GEMM launch ran -- out[9] = BM, BN, K groups, stages, wave multiplier, splits, k_gemm_pp (0 / 1),
// gn_epi (0 none, 1 forward, 2 backward GroupNorm statistics in the epilogue), the split-K reduce left GroupNorm statistics (0 / 1)
extern "C" int dh_dbg_gemm_last_tile(int* out) {
  DH_REQUIRE(out != nullptr, "null pointer");
  const dh::GemmPlan& p = dh::g_last_plan;
  const dh::LaunchedTile& t = dh::g_launched_tile;
  const int v[9] = {t.bm, t.bn, t.kg, t.stages, t.mw, p.splits, p.pp, p.gn_epi, p.reduce == dh::RED_GN_FWD || p.reduce == dh::RED_GN_BWD};
  for (int i = 0; i < 9; ++i) out[i] = v[i];
  return DH_OK;
}

// host-only query of the whole plan (no launch, no device needed): what launch_gemm would decide for the launch `q` describes, under
// the hooks in force.  out[0..22] = the GemmPlan fields in their declared order (gemm_k.h): pp, bm, bn, stages, wg, kg, mw, gm, buf,
// lnf, epi, splits, k_per_split, grid x / y / z, a_bytes, w_bytes, gn_epi, gn_cpg, gn_S, xa, reduce.  tests/test_gemm_plan.py pins
// the table of the SD-2-depth passes on the CPU.
extern "C" int dh_dbg_gemm_plan(const dh_gemm_plan_query* q, int32_t* out, int n_out) {
  using namespace dh;
  static_assert(sizeof(GemmPlan) == GEMM_PLAN_FIELDS * sizeof(int32_t), "GemmPlan is GEMM_PLAN_FIELDS 32-bit fields");
  DH_REQUIRE(q && out && n_out >= GEMM_PLAN_FIELDS, "null pointer, or fewer than 23 output slots");
  DH_REQUIRE(q->M > 0 && q->N > 0 && q->K >= 64 && q->conv >= 0 && q->conv <= 2 && (q->conv == 0 || (q->hw > 0 && (q->stride == 1 || q->stride == 2))),
             "bad shape");
  static __attribute__((aligned(16))) unsigned char dummy[32];
  static int carried;
  void* ptr = (q->flags & DH_GEMM_Q_ALIGNED) ? dummy : dummy + 2;
  float* fptr = reinterpret_cast<float*>(dummy);
  GemmArgs a;
  a.A = ptr; a.W = ptr; a.C = ptr; a.M = q->M; a.N = q->N; a.K = q->K;
  a.mode = q->conv == 0 ? A_DENSE : (q->conv == 1 ? A_CONV3 : A_CONVT2);
  if (q->conv) {
    a.Hin = a.Win = q->hw; a.Cin = q->K / 9; a.stride = q->stride; a.up = q->up;
    a.Hout = a.Wout = q->conv == 2 ? 2 * q->hw : q->hw * (q->up ? 2 : 1) / q->stride;
  }
  a.lda = q->lda > 0 ? q->lda : (q->conv ? q->K / 9 : q->K);
  a.ldc = q->ldc > 0 ? q->ldc : q->N;
  a.partial = q->partial_elems ? fptr : nullptr; a.partial_elems = q->partial_elems;
  if (q->flags & DH_GEMM_Q_BIAS) a.bias = fptr;
  if (q->flags & DH_GEMM_Q_RESIDUAL) { a.R = ptr; a.ldr = q->N; }
  if (q->flags & DH_GEMM_Q_ROWVEC) { a.rowvec = fptr; a.rowvec_ld = q->N; }
  a.act_silu = (q->flags & DH_GEMM_Q_SILU) ? 1 : 0;
  if (q->flags & DH_GEMM_Q_LNF) { a.ln_s = fptr; a.ln_t = fptr; a.ln_stats = fptr; }
  if (q->flags & DH_GEMM_Q_GN_STATS) { a.gn_part = fptr; a.gn_HW = q->gn_HW; a.gn_G = q->gn_G; a.gn_done = &carried; }
  if (q->flags & DH_GEMM_Q_GN_BWD) { a.gnb_x = ptr; a.gnb_ldx = q->N; }
  if (q->flags & DH_GEMM_Q_LN_BWD) { a.lnb_x = ptr; a.lnb_done = &carried; }
  if (q->flags & DH_GEMM_Q_GLU_FWD) { a.glu_y = ptr; a.glu_ldy = q->N / 2; }
  if (q->flags & DH_GEMM_Q_GLU_BWD) { a.glub_x = ptr; a.glub_dx = ptr; a.glub_f = q->glub_f; }
  if (q->flags & (DH_GEMM_Q_XATTN_FWD | DH_GEMM_Q_XATTN_DQ)) {
    a.xa_k = ptr; a.xa_v = ptr; a.xa_o = ptr; a.xa_lse = fptr; a.xa_ldk = q->N; a.xa_ldo = q->N;
    a.xa_Nq = q->xa_Nq; a.xa_Nk = q->xa_Nk; a.xa_H = q->xa_H; a.xa_done = &carried;
  }
  if (q->flags & DH_GEMM_Q_XATTN_DQ) { a.xa_q = ptr; a.xa_dq = ptr; a.xa_ldq = q->N; a.xa_lddq = q->N; }
  const GemmK k = fill_gemm_k(a);
  GemmHooks h = current_hooks();
  h.gn_done = a.gn_done != nullptr; h.lnb_done = a.lnb_done != nullptr; h.xa_done = a.xa_done != nullptr;
  const GemmPlan p = gemm_plan(k, a.partial_elems, h);
  memcpy(out, &p, sizeof(p));
  return DH_OK;
}

// test hook: *last = the last GEMM launch of this thread carried a cross-attention in its epilogue (0 no, 1 forward, 2 dQ), *total = how many
// launches of this thread have since the library was loaded (either pointer may be NULL)
extern "C" int dh_dbg_gemm_xattn_carried(int* last, long long* total) {
  if (last) *last = dh::g_last_plan.xa;
  if (total) *total = dh::g_xattn_total;
  return DH_OK;
}

extern "C" int dh_gemm_profile_begin(void) {
  dh::g_prof.on = true;
  dh::g_prof.used = 0;
  dh::g_prof.flops = 0;
  dh::g_prof.bytes = 0;
  return DH_OK;
}
extern "C" int dh_gemm_profile_bytes(double* bytes) {
  if (bytes) *bytes = dh::g_prof.bytes;
  return DH_OK;
}
extern "C" int dh_gemm_profile_end(double* ms_total, int64_t* launches, double* flops) {
  using namespace dh;
  g_prof.on = false;
  double ms = 0;
  if (g_prof.used >= 2) DH_CHECK_HIP(hipEventSynchronize(g_prof.ev[g_prof.used - 1]));
  for (size_t i = 0; i + 1 < g_prof.used; i += 2) {
    float t = 0;
    DH_CHECK_HIP(hipEventElapsedTime(&t, g_prof.ev[i], g_prof.ev[i + 1]));
    ms += t;
  }
  if (ms_total) *ms_total = ms;
  if (launches) *launches = (int64_t)(g_prof.used / 2);
  if (flops) *flops = g_prof.flops;
  return DH_OK;
}
