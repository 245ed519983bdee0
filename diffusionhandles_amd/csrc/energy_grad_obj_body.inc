// The workgroup body of k_energy_grad_obj / k_energy_grad_obj_batch (included into both, so that the two are one text): the body of
// energy_grad_body.inc with a weight per object.  Expects the arguments of k_energy_grad under their names, with fg_w (the plain
// foreground weight) in place of coef_fg, and objp = the object block of the plan (carve_plan_obj):
//   [0, 32) omega[8] f32 | [32, 64) N[8] i32 | [64, 128) omega / N [8] f64 | [128, ...) the object of every CSR entry
// A segment lists its entries in ascending (object, source cell) order.  Within an object's run the sign sums are integers; when
// the object changes the run is folded into an f32 accumulator with that object's coefficient fg_w * omega_m / (C N_m), written
// as dh_energy_fwd_bwd_planned writes fg_w / (C N): with one object of weight 1 the element is the unweighted kernel's, bit for
// bit.  Fixed order (objects ascending), one writer per element, no atomics: reproducible from run to run.
// DH_ENERGY_SRC(m): the base pointer of the source rows of object m, defined by the including kernel -- orig in the kernels above,
// a select between orig and the donor image's activations by the object's bit in k_energy_grad_donor[_batch].
  __shared__ double sm[4];
  const float* omega = reinterpret_cast<const float*>(objp);
  const int* nobj = reinterpret_cast<const int*>(objp + 32);
  const double* lossw = reinterpret_cast<const double*>(objp + 64);
  const uint8_t* obj = objp + 128;
  const int nch = C / 8, cpb = (int)blockDim.x / nch;
  const int lc = threadIdx.x / nch, ch = threadIdx.x - lc * nch;
  const int cell = blockIdx.x * cpb + lc;
  double la = 0.0, lb = 0.0;
  // prologue: energy_grad_body.inc's (sign of the difference of the two background means from the quarter sums of k_colsum_q)
  float sgn[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) sgn[i] = 0.f;
  if (use_bg && lc < cpb) {
    float qa[4][8], qb[4][8];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      *reinterpret_cast<float4*>(&qa[q][0]) = *reinterpret_cast<const float4*>(partq + (size_t)q * C + ch * 8);
      *reinterpret_cast<float4*>(&qa[q][4]) = *reinterpret_cast<const float4*>(partq + (size_t)q * C + ch * 8 + 4);
      *reinterpret_cast<float4*>(&qb[q][0]) = *reinterpret_cast<const float4*>(partq + (size_t)(4 + q) * C + ch * 8);
      *reinterpret_cast<float4*>(&qb[q][4]) = *reinterpret_cast<const float4*>(partq + (size_t)(4 + q) * C + ch * 8 + 4);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float a = ((qa[0][i] + qa[1][i]) + qa[2][i]) + qa[3][i];
      const float b = ((qb[0][i] + qb[1][i]) + qb[2][i]) + qb[3][i];
      const float d = a / (float)n1 - b / (float)n2;
      sgn[i] = (float)((d > 0.f) - (d < 0.f));
      if (blockIdx.x == 0 && lc == 0) lb += (double)fabsf(d);
    }
  }
  if (lc < cpb && cell < G2) {
    const uint4 ra = *reinterpret_cast<const uint4*>(cur + (size_t)cell * C + ch * 8);
    const T* av = reinterpret_cast<const T*>(&ra);
    float a[8], gf[8];
    int sg[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) { a[i] = to_f32<T>(av[i]); sg[i] = 0; gf[i] = 0.f; }
    const int b = off[cell], e = b + ucnt[cell];
    int m = b < e ? (int)obj[b] : 0;          // the object of the current run
    double lr = 0.0;                          // sum of mult |d| over the run
// closes the run of object m
#define DH_FOLD_OBJECT()                                                              \
  do {                                                                                \
    const float cm = fg_w * (omega[m] * (1.f / ((float)C * (float)nobj[m])));         \
    _Pragma("unroll") for (int i = 0; i < 8; ++i) { gf[i] += cm * (float)sg[i]; sg[i] = 0; } \
    la += lossw[m] * lr;                                                              \
    lr = 0.0;                                                                         \
  } while (0)
    int k = b;
    for (; k + 8 <= e; k += 8) {        // 8 distinct source rows in flight
      int id[8], mu[8], ob[8];
      uint4 ro[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) { id[j] = src[k + j]; mu[j] = mult[k + j]; ob[j] = (int)obj[k + j]; }
#pragma unroll
      for (int j = 0; j < 8; ++j) ro[j] = *reinterpret_cast<const uint4*>(DH_ENERGY_SRC(ob[j]) + (size_t)id[j] * C + ch * 8);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (ob[j] != m) { DH_FOLD_OBJECT(); m = ob[j]; }
        const T* ov = reinterpret_cast<const T*>(&ro[j]);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const float d = to_f32<T>(ov[i]) - a[i];
          lr += (double)mu[j] * (double)fabsf(d);
          sg[i] += mu[j] * ((d > 0.f) - (d < 0.f));
        }
      }
    }
    for (; k < e; ++k) {
      const int mu = mult[k], ob = (int)obj[k];
      const uint4 ro = *reinterpret_cast<const uint4*>(DH_ENERGY_SRC(ob) + (size_t)src[k] * C + ch * 8);
      if (ob != m) { DH_FOLD_OBJECT(); m = ob; }
      const T* ov = reinterpret_cast<const T*>(&ro);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float d = to_f32<T>(ov[i]) - a[i];
        lr += (double)mu * (double)fabsf(d);
        sg[i] += mu * ((d > 0.f) - (d < 0.f));
      }
    }
    if (b < e) DH_FOLD_OBJECT();
#undef DH_FOLD_OBJECT
    const bool bg = use_bg && bgflag[cell];
    TG o[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      float g = 0.f;
      if (b < e) g += -gf[i];
      if (bg) g += -coef_bg * sgn[i];
      o[i] = from_f32<TG>(g * scale);
    }
    if (sizeof(TG) == 2) {
      *reinterpret_cast<uint4*>(grad + (size_t)cell * C + ch * 8) = *reinterpret_cast<uint4*>(o);
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) grad[(size_t)cell * C + ch * 8 + i] = o[i];
    }
  }
  la = block_sum(la, sm);
  if (threadIdx.x == 0) loss_part[blockIdx.x] = la;
  if (blockIdx.x == 0 && use_bg) {
    lb = block_sum(lb, sm);
    if (threadIdx.x == 0) bg_loss[0] = lb;
  }
