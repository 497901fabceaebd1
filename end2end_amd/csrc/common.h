// Shared helpers for the MI355X (gfx950) CTC library.  Wave size is 64.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <math.h>

#include "../../include/e2e_ctc.h"
#include "../../include/e2e_ctc_debug.h"

namespace e2e {

constexpr int kWave = 64;

// 16-bit I/O types of the kernels (E2E_F16 / E2E_BF16): plain arithmetic types of the compiler, converted on load / store
typedef _Float16 f16_t;
typedef __bf16 bf16_t;
inline bool dtype_is_16bit(int dtype) { return dtype == E2E_F16 || dtype == E2E_BF16; }
// losses / reduced of a call: the I/O dtype, except that 16-bit calls keep them in f32 (include/e2e_ctc.h)
template <typename IO> struct LossOf { typedef IO type; };
template <> struct LossOf<f16_t> { typedef float type; };
template <> struct LossOf<bf16_t> { typedef float type; };
// one element of a tensor whose dtype is known at run time only (wave-uniform `dt`): used where a kernel is not worth an
// instance per dtype
__device__ __forceinline__ float load_elem(const void* base, int64_t idx, int dt) {
  if (dt == E2E_F32) return reinterpret_cast<const float*>(base)[idx];
  if (dt == E2E_BF16) return (float)reinterpret_cast<const bf16_t*>(base)[idx];
  return (float)reinterpret_cast<const f16_t*>(base)[idx];
}
__device__ __forceinline__ void store_elem(void* base, size_t idx, float v, int dt) {
  if (dt == E2E_F32) reinterpret_cast<float*>(base)[idx] = v;
  else if (dt == E2E_BF16) reinterpret_cast<bf16_t*>(base)[idx] = (bf16_t)v;
  else reinterpret_cast<f16_t*>(base)[idx] = (f16_t)v;
}

// A target as the lattice kernels hold it, an int: -1 (outside every alphabet) unless the int64 lies in [0, 2^32) -- its upper
// word is tested BEFORE it is narrowed, so that 2^32 + 3 or 3 - 2^32 never becomes label 3 (values of 2^31 .. 2^32 - 1 come out
// negative, outside the alphabet as well).  One compare and one select per label read.
__device__ __forceinline__ int label_of(int64_t v) { return (v >> 32) != 0 ? -1 : (int)v; }

// thread-local error text behind e2e_last_error()
void set_error(const char* fmt, ...);
int hip_fail(hipError_t e, const char* what);

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
// A caller's workspace starts at any address; the kernels' buffers at the first 256-byte boundary in it.
inline unsigned char* aligned_256(const void* p) {
  return reinterpret_cast<unsigned char*>((reinterpret_cast<uintptr_t>(p) + 255) & ~(uintptr_t)255);
}
// `ws` to that boundary and `bytes` to what is left behind it; false (both unchanged) for no workspace or one that ends before it
inline bool align_workspace(void*& ws, size_t& bytes) {
  const size_t pad = aligned_256(ws) - reinterpret_cast<unsigned char*>(ws);
  if (!ws || bytes < pad) return false;
  ws = aligned_256(ws); bytes -= pad;
  return true;
}
// the reduction of an e2e_ctc_loss_opts (null: defaults) is one of E2E_REDUCE_* and has somewhere to go; else sets the error
inline bool loss_opts_ok(const e2e_ctc_loss_opts* opts) {
  if (!opts || (opts->reduction >= E2E_REDUCE_NONE && opts->reduction <= E2E_REDUCE_MEAN &&
                (opts->reduction == E2E_REDUCE_NONE || opts->reduced))) return true;
  set_error("bad e2e_ctc_loss_opts: reduction %d, reduced %p", opts->reduction, opts->reduced);
  return false;
}

__device__ __forceinline__ double ninf() { return -__builtin_huge_val(); }

// the reference's two-argument log-sum-exp, src/utils/math_utils.h:8-16 (log(1.0 + x), not log1p)
__device__ __forceinline__ double lse2(double a, double b) {
  if (a == ninf()) return b;
  if (b == ninf()) return a;
  if (a > b) return a + log(1.0 + exp(b - a));
  return b + log(1.0 + exp(a - b));
}

// hipFuncAttributeMaxDynamicSharedMemorySize = `bytes` for kernel `fn`, raised when a launch needs more than the largest size asked for so far per (kernel, device) --
// not on every launch: a host call that an entry point meant to be captured into a graph should not repeat.  Returns a hipError_t.
hipError_t allow_dynamic_lds(const void* fn, int bytes);

// -- launchers implemented in the .hip files ---------------------------------
struct LossArgs {
  const void* x; int dtype; int logprobs;
  int64_t sB, sT, sV;
  const int64_t* targets; int64_t tgt_stride;
  const int64_t* x_len; const int64_t* t_len;
  int B, T, V, Smax, blank;
  void* losses; void* grads;
  void* ws; size_t ws_bytes;
  hipStream_t stream;
  // e2e_ctc_loss_opts (include/e2e_ctc.h): every gradient element is multiplied by grad_scale as it is written;
  // `reduced` (one element of the I/O dtype, may be null) receives the sum / mean of the B losses
  double grad_scale = 1.0;
  void* reduced = nullptr;
  int reduction = 0;
  int chains = 0;          // E2E_CHAINS_*
  int scaled_exact = 0;    // the exact kernel may use its scaled probability-domain form (f32 I/O, algo AUTO; see ctc_exact_one)
};
// sum / mean of the losses by one small launch (paths that have no tail to fold it into)
int launch_reduce_losses(const LossArgs& a);

// Exponential tilt of the fast path's scaled lattice (rows hold alpha[j] r^j and beta[j] r^(L-1-j)); shared by the
// kernels that produce and that consume its checkpoints.  See LaneCells in ctc_loss_fast.hip.
// frame number -> (utterance, step) for the one-wave-per-frame kernels: a 32-bit division where the frame count allows it
// (a 64-bit one is ~100 instructions, more than some of those kernels' own work per frame)
__device__ __forceinline__ void split_frame(int64_t row, int T, int& b, int& t) {
  if (row < 0x7fffffffLL) { const unsigned r = (unsigned)row, q = r / (unsigned)T; b = (int)q; t = (int)(r - q * (unsigned)T); }
  else { b = (int)(row / T); t = (int)(row - (int64_t)b * T); }
}

__host__ __device__ inline float fast_tilt(int S, int T) {
  float rho = (float)S / (float)T;
  rho = fminf(fmaxf(rho, 1.f / 33.f), 0.8f);
  return S > 0 ? 2.f * rho / (1.f - rho) : 1.f;
}
constexpr int kFastSeg = 16;       // steps between two checkpoints of the fast path

// What the flagged-utterance launch needs to redo only the SECOND kernel of the fast path in f64 (an utterance whose
// f32 segment kernel ran out of range keeps its f64 chains' results: checkpoints, probabilities, loss).
struct FastRetry {
  int* ctl;                        // the fast path's control words (see FastParams::ctl)
  int ytab_segments;               // ytab is [B][NS][V][16] (the small alphabets' form) instead of [B][T][V]
  const float* ytab; const float* ckA; const float* ckQ; const short* ckE; const int* cumA; const int* cumB;
  const double* logz;              // [B][2] the chains' log Z (alpha side, beta side)
  const unsigned* segmask;         // [B][MW] bit s: segment s failed its range / self-check in the segment kernel (only those are redone)
  int NS, NB, CELLS, PPL, MW;
  // the extended-range redo (ctc_ext.h): per-cell exponents of the checkpoint rows it writes over ckA / ckQ for the
  // utterances it takes, and their partition sums
  int* ckXA; int* ckXQ;            // [B][NS][CELLS]
  double* extz;                    // [B][2]  Z = extz[0] * 2^extz[1]; behind them [B][2 sides][4]: the sides' cells of Z when alpha and beta ran on two workgroups
};

size_t exact_workspace_bytes(int B, int T, int V, int Smax);            // every utterance (algo EXACT)
size_t exact_fallback_workspace_bytes(int B, int T, int V, int Smax);   // flagged-utterance fallback of the fast path
int launch_exact(const LossArgs& a);
size_t fast_workspace_bytes(int B, int T, int V, int Smax);
int launch_fast(const LossArgs& a, bool fallback_to_exact);
bool fast_supported(int T, int V, int Smax, int dtype);
// what a fast-path call of this shape runs, for e2e_debug_loss_route: 10 * pairs per lane + the number of the rule of
// launch_fast_ppl's list that picks its chains (computed by the function the launch follows); 0: not a shape of the fast path
int fast_route(int B, int V, int Smax, int chains);
// wide alphabets: per-utterance compaction around the fast path (ctc_loss_wide.hip)
bool wide_supported(int T, int V, int Smax, int dtype);
bool wide_takes_fast_lattice(int T, int V, int Smax, int dtype);   // (false: the compact lattice is the exact kernel's)
size_t wide_workspace_bytes(int B, int T, int V, int Smax, bool with_exact);
int launch_wide(const LossArgs& a, bool fallback_to_exact);
// the wide path's row kernels for these logits (launch_wide follows it): 0 element by element in two passes, 1 the same by
// 16-byte accesses, 2 / 3 / 4 the single-read kernels of 8 / 16 / 32 accesses per lane (rows of up to 2048 / 4096 / 8192 columns)
int wide_row_form(int dtype, int V, int64_t sB, int64_t sT, int64_t sV, const void* x, const void* grads);

}  // namespace e2e

#define E2E_HIP_CHECK(expr, what)                          \
  do {                                                     \
    hipError_t _e = (expr);                                \
    if (_e != hipSuccess) return e2e::hip_fail(_e, what);  \
  } while (0)
