// What the blank-free and Gram-CTC losses (ctc_loss_noblank.hip, ctc_loss_gram.hip) share: one numeric scheme and one
// call shape around two lattice recurrences that genuinely differ.
//   device  the row pass (one wave per frame: the row's log-sum-exp and the dense part of the gradient), the wave
//           reductions, the power-of-two row scaling, the thresholds that send an f32 utterance to the log domain, the
//           settle step at the end of the forward sweep;
//   host    the workspace layout, the argument checks of the two entry points, the two launches with the optional
//           reduction behind them, and the reader of the redo flags.
// P is the calling file's parameter block.  Every helper that receives it is __forceinline__: a block handed by
// reference to a function the compiler does not inline is copied to scratch at the kernel's entry
// (tools/perf/entry_audit.py).
#pragma once
#include "common.h"

namespace e2e {

constexpr int kLatticeThreads = 256;         // one workgroup per utterance
constexpr double kLowLp = -700.0;            // a finite log-probability below this sends an f32 utterance to the log domain
// Every frame's posteriors sum to 1.  A row is scaled by its LARGEST cell, and a cell far below it that still carries
// paths can flush to zero; the mass it carried is then missing from its frame's sum.  Beta checks every frame's sum;
// an utterance whose sum is off by more than kMassTol is redone in the log domain after the backward sweep (the redo
// rewrites every label column it wrote).
constexpr double kMassTol = 1e-9;
constexpr double kLn2 = 0.69314718055994530942;

__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_lse(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = lse2(v, __shfl_xor(v, o, 64));
  return v;
}
// biased exponent of a non-negative double (0: zero or subnormal, 2047: inf / NaN)
__device__ __forceinline__ int expo(double a) { return (__double2hiint(a) >> 20) & 0x7ff; }
// 2^(1023 - m): divides a row whose largest biased exponent is m into [1, 2)
__device__ __forceinline__ double inv_pow2(int m) { return __hiloint2double((2046 - m) << 20, 0); }
// a row's largest biased exponent left the range inv_pow2 serves: the row is all zero / subnormal, or it overflowed
__device__ __forceinline__ bool expo_out_of_range(int m) { return m == 0 || m >= 2046; }

// The end of a probability-domain forward sweep (a barrier: every thread calls it).  Does the utterance go to the log
// domain -- a row left the exponent range, a gather met a log-probability below kLowLp, or the scaled total zm is not a
// positive finite number?  If not, log Z from zm and the exponents summed over the rows.  (By reference, so that the
// operands are read where the expression reads them: by value the f32 lattice kernels come out differently scheduled.)
__device__ __forceinline__ int prob_unsettled(const int& range_bad, const int& low_lp, const double& zm) {
  return __syncthreads_or(range_bad || low_lp || !(zm > 0.0) || !(zm < INFINITY));
}
__device__ __forceinline__ double prob_log_z(double zm, int cend) { return log(zm) + (double)cend * kLn2; }

// The row pass: needs x, sB, sT, sV, x_len, B, T, V, logits, gscale and grads of P.
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

// ---- lattice_host: the call around the two kernels ----

// Workspace (offsets from its 256-byte aligned start): lse [B][T] f64, ck [B][NB][cells] f64 alpha checkpoint rows,
// ckc [B][NB] their exponents, redo [B].  K is the LDS block in frames (0: no block of rows this wide fits, and the
// layout is empty); a checkpoint is kept every `ck_frames` frames.
struct LatticeLayout { size_t lse, ck, ckc, redo, total; int K, NB, cells; };
inline LatticeLayout lattice_layout(int B, int T, int cells, int K, int ck_frames) {
  LatticeLayout l{};
  if (K == 0) return l;
  l.K = K; l.cells = cells;
  l.NB = (T + ck_frames - 1) / ck_frames;
  l.lse = 0;
  l.ck = align_up((size_t)B * T * sizeof(double), 256);
  l.ckc = l.ck + align_up((size_t)B * l.NB * cells * sizeof(double), 256);
  l.redo = l.ckc + align_up((size_t)B * l.NB * sizeof(int), 256);
  l.total = l.redo + align_up((size_t)B * sizeof(int), 256);
  return l;
}

// The checks both entry points make of the arguments they share; takes the options into `a`.
inline int lattice_check_args(LossArgs& a, const e2e_ctc_loss_opts* opts) {
  if (a.dtype != E2E_F32 && a.dtype != E2E_F64) { set_error("dtype must be E2E_F32 or E2E_F64 (up-cast 16-bit inputs)"); return E2E_ERR_ARG; }
  if (a.B < 0 || a.T < 1 || a.V < 1 || a.Smax < 0) { set_error("bad sizes B=%d T=%d V=%d Smax=%d", a.B, a.T, a.V, a.Smax); return E2E_ERR_ARG; }
  if (!loss_opts_ok(opts)) return E2E_ERR_ARG;
  if (a.B > 0 && (!a.x || !a.x_len || !a.t_len || !a.losses || !a.grads || !a.targets)) { set_error("null pointer argument"); return E2E_ERR_ARG; }
  if (opts) { a.grad_scale = opts->grad_scale; a.reduced = opts->reduced; a.reduction = opts->reduction; }
  return E2E_OK;
}

// a.ws becomes the aligned start of the caller's workspace, which must hold the layout behind it
inline int lattice_workspace(LossArgs& a, const LatticeLayout& l) {
  size_t left = a.ws_bytes;
  if (!align_workspace(a.ws, left) || left < l.total) { set_error("workspace too small: need %zu", l.total + 256); return E2E_ERR_WORKSPACE; }
  return E2E_OK;
}

// the fields every parameter block has
template <typename P>
void lattice_params(P& p, const LossArgs& a, const LatticeLayout& l) {
  unsigned char* ws = reinterpret_cast<unsigned char*>(a.ws);
  p.x = a.x; p.sB = a.sB; p.sT = a.sT; p.sV = a.sV;
  p.targets = a.targets; p.tgt_stride = a.tgt_stride; p.x_len = a.x_len; p.t_len = a.t_len;
  p.B = a.B; p.T = a.T; p.V = a.V; p.Smax = a.Smax; p.logits = a.logprobs ? 0 : 1; p.K = l.K; p.NB = l.NB;
  p.gscale = a.grad_scale; p.losses = a.losses; p.grads = a.grads;
  p.lse = reinterpret_cast<const double*>(ws + l.lse); p.ck = reinterpret_cast<double*>(ws + l.ck); p.ckc = reinterpret_cast<int*>(ws + l.ckc);
}

// The f32 and f64 instances of a file's two kernels (X: what its lattice kernel takes behind the block) and their names
// in an error text.
template <typename P, typename... X>
struct LatticeKernels {
  void (*rows32)(P, double*); void (*rows64)(P, double*); const char* rows_launch;
  void (*lattice32)(P, X...); void (*lattice64)(P, X...); const char* lattice_launch;
};

// The row pass, the lattice with `lds` bytes of dynamic LDS, and the sum / mean of the losses if the call asks for one.
template <typename P, typename... X>
int lattice_launch(const LossArgs& a, const LatticeKernels<P, X...>& k, const P& p, size_t lds, X... extra) {
  const bool f32 = a.dtype == E2E_F32;
  const unsigned rows_grid = (unsigned)(((int64_t)a.B * a.T + 3) / 4);
  double* lse_out = const_cast<double*>(p.lse);       // (the row pass writes what the lattice reads)
  hipLaunchKernelGGL(f32 ? k.rows32 : k.rows64, dim3(rows_grid), dim3(256), 0, a.stream, p, lse_out);
  E2E_HIP_CHECK(hipGetLastError(), k.rows_launch);
  const auto lattice = f32 ? k.lattice32 : k.lattice64;
  E2E_HIP_CHECK(allow_dynamic_lds(reinterpret_cast<const void*>(lattice), (int)lds), "hipFuncSetAttribute");
  hipLaunchKernelGGL(lattice, dim3(a.B), dim3(kLatticeThreads), lds, a.stream, p, extra...);
  E2E_HIP_CHECK(hipGetLastError(), k.lattice_launch);
  return launch_reduce_losses(a);
}

// the redo flags of the last call with this workspace, to the host (synchronises)
inline int lattice_redo_flags(const void* workspace, const LatticeLayout& l, int B, int* flags_host) {
  if (l.K == 0) { set_error("no such layout"); return E2E_ERR_UNSUPPORTED; }
  E2E_HIP_CHECK(hipDeviceSynchronize(), "hipDeviceSynchronize");
  E2E_HIP_CHECK(hipMemcpy(flags_host, aligned_256(workspace) + l.redo, sizeof(int) * B, hipMemcpyDeviceToHost), "hipMemcpy");
  return E2E_OK;
}

}  // namespace e2e
