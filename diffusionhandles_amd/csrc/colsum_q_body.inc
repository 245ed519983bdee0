// The workgroup body of k_colsum_q / k_colsum_q_batch (included into both, so that the two are one text): expects
// z (list 0 / 1), X, list, n of that list, C, and partq = the item's [2][4][C] table.
  __shared__ float sp[CQ_SL][8][8];
  const int q = blockIdx.y, sloc = threadIdx.x >> 3, cl = threadIdx.x & 7;
  const int ch = blockIdx.x * 8 + cl;                       // 8-channel chunk
  const int sl = q * CQ_SL + sloc;
  const int per = (n + COLSUM_S - 1) / COLSUM_S, b = sl * per, e = b + per < n ? b + per : n;
  float acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = 0.f;
  if (ch * 8 < C) {
    int k = b;
    for (; k + 16 <= e; k += 16) {          // 16 gathers in flight; the adds keep the list order
      int id[16];
      uint4 raw[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) id[j] = list[k + j];
#pragma unroll
      for (int j = 0; j < 16; ++j) raw[j] = *reinterpret_cast<const uint4*>(X + (size_t)id[j] * C + ch * 8);
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const T* v = reinterpret_cast<const T*>(&raw[j]);
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] += to_f32<T>(v[i]);
      }
    }
    if (k + 8 <= e) {
      int id[8];
      uint4 raw[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) id[j] = list[k + j];
#pragma unroll
      for (int j = 0; j < 8; ++j) raw[j] = *reinterpret_cast<const uint4*>(X + (size_t)id[j] * C + ch * 8);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const T* v = reinterpret_cast<const T*>(&raw[j]);
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] += to_f32<T>(v[i]);
      }
      k += 8;
    }
    for (; k < e; ++k) {
      const uint4 raw = *reinterpret_cast<const uint4*>(X + (size_t)list[k] * C + ch * 8);
      const T* v = reinterpret_cast<const T*>(&raw);
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[i] += to_f32<T>(v[i]);
    }
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) sp[sloc][cl][i] = acc[i];
  __syncthreads();
  if (threadIdx.x < 64) {                   // (chunk, channel): the quarter's slices in slice order
    const int c2 = threadIdx.x >> 3, i = threadIdx.x & 7;
    float a = 0.f;
    for (int s = 0; s < CQ_SL; ++s) a += sp[s][c2][i];
    const int c = (blockIdx.x * 8 + c2) * 8 + i;
    if (c < C) partq[((size_t)z * 4 + q) * C + c] = a;
  }
