// The workgroup body of k_energy_grad / k_energy_grad_batch (included into both, so that the two are one text): expects the
// arguments of k_energy_grad under their names.
  __shared__ double sm[4];
  const int nch = C / 8, cpb = (int)blockDim.x / nch;
  const int lc = threadIdx.x / nch, ch = threadIdx.x - lc * nch;
  const int cell = blockIdx.x * cpb + lc;
  double la = 0.0, lb = 0.0;
  // prologue: sign of the difference of the two background means of this thread's 8 channels from the quarter sums of k_colsum_q
  // (a 2 x 4 x C f32 table, L2-resident; every lane of a chunk reads the same 16 sectors) -- the arithmetic of k_global_diff
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
      if (blockIdx.x == 0 && lc == 0) lb += (double)fabsf(d);          // the loss of the term: once, by the first cell's lanes of block 0
    }
  }
  if (lc < cpb && cell < G2) {
    const uint4 ra = *reinterpret_cast<const uint4*>(cur + (size_t)cell * C + ch * 8);
    const T* av = reinterpret_cast<const T*>(&ra);
    float a[8];
    int sg[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) { a[i] = to_f32<T>(av[i]); sg[i] = 0; }
    const int b = off[cell], e = b + ucnt[cell];
    int k = b;
    for (; k + 8 <= e; k += 8) {        // 8 distinct source rows in flight
      int id[8], mu[8];
      uint4 ro[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) { id[j] = src[k + j]; mu[j] = mult[k + j]; }
#pragma unroll
      for (int j = 0; j < 8; ++j) ro[j] = *reinterpret_cast<const uint4*>(orig + (size_t)id[j] * C + ch * 8);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const T* ov = reinterpret_cast<const T*>(&ro[j]);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const float d = to_f32<T>(ov[i]) - a[i];
          la += (double)mu[j] * (double)fabsf(d);
          sg[i] += mu[j] * ((d > 0.f) - (d < 0.f));
        }
      }
    }
    for (; k < e; ++k) {
      const uint4 ro = *reinterpret_cast<const uint4*>(orig + (size_t)src[k] * C + ch * 8);
      const int mu = mult[k];
      const T* ov = reinterpret_cast<const T*>(&ro);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float d = to_f32<T>(ov[i]) - a[i];
        la += (double)mu * (double)fabsf(d);
        sg[i] += mu * ((d > 0.f) - (d < 0.f));
      }
    }
    const bool bg = use_bg && bgflag[cell];
    TG o[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      float g = 0.f;
      if (b < e) g += -coef_fg * (float)sg[i];
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
