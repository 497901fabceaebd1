// The row pass of the blank-free and Gram-CTC losses (ctc_loss_noblank.hip, ctc_loss_gram.hip): one wave per frame, the
// row's log-sum-exp (logits in: log-softmax fused; kept in the workspace) and the dense part of the gradient,
// grad[t, v] = scale * exp(lp[t, v]), 0 on padded frames.  P is the calling file's parameter block: it needs x, sB, sT, sV,
// x_len, B, T, V, logits, gscale and grads.
#pragma once
#include "common.h"

namespace e2e {

template <typename IO, typename P>
__device__ __forceinline__ void loss_rows(const P& p, double* lse_out) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= (int64_t)p.B * p.T) return;
  const int b = (int)(row / p.T), t = (int)(row - (int64_t)b * p.T);
  const int V = p.V;
  IO* g = reinterpret_cast<IO*>(p.grads) + row * V;
  const int64_t xl = p.x_len[b];
  if (t >= xl) {                              // padded frame (and every frame of a bad length: the lattice writes its NaN slab)
    for (int v = lane; v < V; v += 64) g[v] = (IO)0;
    return;
  }
  const IO* x = reinterpret_cast<const IO*>(p.x) + (int64_t)b * p.sB + (int64_t)t * p.sT;
  double lse = 0.0;
  if (p.logits) {
    double m = ninf();
    for (int v = lane; v < V; v += 64) m = fmax(m, (double)x[(int64_t)v * p.sV]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o, 64));
    double s = 0.0;
    for (int v = lane; v < V; v += 64) s += exp((double)x[(int64_t)v * p.sV] - m);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    lse = m + log(s);
    if (lane == 0) lse_out[row] = lse;
  }
  for (int v = lane; v < V; v += 64) g[v] = (IO)(p.gscale * exp((double)x[(int64_t)v * p.sV] - lse));
}

}  // namespace e2e
