/* Diagnostics of libe2e_ctc.so -- NOT part of the drop-in contract (that is include/e2e_ctc.h).
 *
 * These entry points exist so that bench.py and tools/diag/ can look inside a call without a second
 * library: they synchronise the device and copy small records to the host, so they never belong in a
 * training step.  A caller that only wants the reference's behaviour never needs this header.
 * Every exported e2e_* symbol of the library is declared in one of the two headers
 * (tests/test_host_cpu.py checks both directions).
 */
#ifndef E2E_CTC_DEBUG_H
#define E2E_CTC_DEBUG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* dst[0..bytes) = src[0..bytes) by a plain streaming kernel on `stream` (bytes % 16 == 0): the on-box
 * copy rate bench.py reports as roofline.peak_measured beside the 8 TB/s spec. */
int e2e_debug_stream_copy(void* dst, const void* src, size_t bytes, void* stream);

/* Keeps `workgroups` workgroups of `threads` threads, each holding `lds_bytes` of LDS, resident for `nanoseconds` (<= 0.1 s) on
 * `stream`, doing nothing: tests/test_gpu_fuzz.py runs the loss call's flagged launch beside it (its bounded waits must end in
 * right results whether they run out or not). */
int e2e_debug_occupy(int workgroups, int threads, int lds_bytes, long long nanoseconds, void* stream);

/* Which kernels e2e_ctc_loss_fwd_bwd_opt gives a call of these sizes, strides and pointers (`chains`: e2e_ctc_loss_opts.chains),
 * computed on the host by the functions the call itself dispatches with; no GPU is touched.  -1: the call is refused (bad
 * sizes, a shape E2E_ALGO_FAST does not take, 16-bit logits the caller has to up-cast).  Otherwise 1000 * path + 100 * rows +
 * 10 * pairs + rule:
 *   path   1 the exact kernel (rows, pairs, rule 0); 2 the fast path; 3 the wide path (per-utterance compact alphabet of Smax + 1
 *          columns) with the fast path's lattice on it; 4 the wide path with the exact kernel's lattice (rows only)
 *   rows   the wide path's row kernels: 0 element by element in two passes, 1 the same by 16-byte accesses, 2 / 3 / 4 the
 *          single-read kernels for up to 2048 / 4096 / 8192 columns; 0 on the other paths
 *   pairs  label pairs per lane of the lattice kernels: 1, 2, 4, 8 (targets tensors of up to 63 / 127 / 255 / 447 columns;
 *          alphabets of 97..224 columns 4 up to 223 labels, 8 beyond; of 225..448 columns always 8)
 *   rule   what picks the chain kernel, as listed at launch_fast_ppl (end2end_amd/csrc/ctc_loss_fast.hip): 1 the wide-row forms
 *          behind a probability table, 2 ChainF64L (eight pairs), 3 ChainF32, 4 the lean halo chains, 5 ChainF64, 6 the single-wave
 *          chains, 7 the same with the ring of four blocks (B > 256)
 * It is the WIDTH of the targets tensor, Smax, that selects all this -- not the longest target in it. */
int e2e_debug_loss_route(int dtype, int algo, int B, int T, int V, int Smax, int chains,
                         int64_t sB, int64_t sT, int64_t sV, const void* x, const void* grads);

/* Whether the producers of the lean halo chain kernel (rule 4 above) take logits of this dtype, frame count, alphabet and
 * strides by their lean form -- an utterance's base address plus 32-bit byte offsets -- (1) or keep 64-bit offsets (0): the
 * host's choice, computed by the function the launch follows; no GPU is touched.  1 needs f32, sV == 1, 0 <= sT < 2^22,
 * 1 <= T < 2^24, and ((T - 1) sT + V + 8) * 4 as well as an utterance's part of the probability table,
 * ceil(T / 16) * 16 * V * 4 bytes, below 2^31. */
int e2e_debug_chain_lean_input(int dtype, int T, int V, int64_t sT, int64_t sV);

/* After an e2e_ctc_loss_fwd_bwd(ALGO_AUTO / ALGO_FAST) call that took the fast path: the per-utterance
 * flag words (0 = served by the fast path; bits: 1 bad lengths, 2 blank in targets, 4 infeasible,
 * 8 range / self-check, 16 non-finite, 32 log Z mismatch, 64 emissions near the end of f32) and the
 * alpha-side / beta-side log Z of the chains, read out of `workspace`.  Synchronises.
 * The words carry three more bits, which send the utterance to the full recomputation like 1 and 2: 128 a bounded wait
 * inside a chain kernel ran out, 256 a probability below f32's smallest normal number (the fast path's table holds a marker in
 * its place), 512 set by the flagged launch itself: an f64 redo of one of the utterance's segments failed (settled by the
 * extended-range redo's second round).  What the flagged launch does with a word f: nothing for 0; f & (1 | 2 | 128 | 256):
 * full recomputation by the exact kernel; else f & (4 | 32 | 64): the extended-range redo; else (8 / 16 only): the f64 redo of
 * the flagged segments -- unless another utterance of the call takes the extended-range redo, which these then join.
 * The extended-range redo leaves its own marks in the word: 2048 it ran the utterance's chains, 4096 and could not settle it
 * (the exact kernel recomputes it), 8192 / 16384 the alpha / the beta chains have finished on a workgroup of their own. */
int e2e_debug_fast_state(const void* workspace, int B, int T, int V, int Smax, int* flags_host, double* logz_host);

/* How many flagged utterances of that call the f64 redo of the segments could not settle (they were
 * recomputed by the exact kernel).  Synchronises. */
int e2e_debug_fast_redo_failures(const void* workspace, int B, int T, int V, int Smax, int* count_host);

/* After an e2e_gram_ctc_fwd_bwd call with this workspace and these sizes: per utterance, why it was redone in the f64 log
 * domain (0 it was not, or the input was f64; 1 the probability-domain forward could not settle it, an infeasible utterance
 * included; 2 the backward found a frame whose posteriors do not sum to 1, or a beta row out of range).  Synchronises. */
int e2e_debug_gram_redo_flags(const void* workspace, int B, int T, int Smax, int max_order, int* flags_host);

/* The same after an e2e_ctc_noblank_fwd_bwd call with this workspace and these sizes (0 also for an utterance with no lattice
 * to run: bad lengths or labels, or more labels than frames; 1 the probability-domain forward could not settle it; 2 the
 * backward found a frame whose posteriors do not sum to 1, or a beta row out of range).  Synchronises. */
int e2e_debug_noblank_redo_flags(const void* workspace, int B, int T, int Smax, int* flags_host);

/* The flagged-utterance launch of that call as its workgroup 0 saw it, microseconds since the launch's start (100 MHz clock):
 * us[0] end of its f64 redos of single segments, [1] of the wait for the other workgroups, [2] of its extended-range chains,
 * [3] of its extended-range segments, [4] end of the launch's last workgroup, [5] when that workgroup learnt it was the last
 * (us_host holds six).  Zeros when nothing was flagged.  Synchronises. */
int e2e_debug_flagged_phases(const void* workspace, int B, int T, int V, int Smax, double* us_host);

/* Bounded waits of that call's flagged-utterance launch that ran out (0 on an idle GPU; what they left undone was recomputed by the
 * exact kernel) and f64 redos of single segments that failed (handed to the extended-range redo).  Synchronises. */
int e2e_debug_flagged_counters(const void* workspace, int B, int T, int V, int Smax, int* timeouts_host, int* failed_redos_host);

/* Segments of that call whose window of posterior mass did not fit the banded segment kernel's 128 label pairs (targets tensors
 * of 128..255 columns): they set flag 8 and were redone in f64 by the flagged launch.  Synchronises. */
int e2e_debug_band_misses(const void* workspace, int B, int T, int V, int Smax, int* count_host);

/* Which segment kernel the calls that follow run behind the chains of targets tensors of 128..255 columns (alphabets of up to 96
 * columns): 1 (the default) the banded form, two label pairs per lane over the 128 pairs that carry the segment's posterior
 * mass; 0 the four-pair instance over the whole lattice.  Any other value changes nothing.  Returns the previous setting.
 * A process-wide switch for A/B timing (tools/diag); not synchronised with calls in flight on other threads. */
int e2e_debug_segment_band(int on);

#ifdef E2E_FAST_PROFILE   /* only in builds made by tools/diag/build_profile_lib.sh */
int e2e_debug_fast_zdev(float* host, int reset);
int e2e_debug_fast_profile(unsigned long long* host, int n);
int e2e_debug_fast_profile2(unsigned long long* host, int reset);
int e2e_debug_fast_profile3(unsigned long long* host, int reset);
#endif
#ifdef E2E_BEAM_PROFILE
int e2e_debug_beam_profile(unsigned long long* host);
int e2e_debug_beam_sigs(unsigned long long* host, int cap);   /* LM states of utterance 0 that had to ask, in order; resets the list */
#endif

#ifdef __cplusplus
}
#endif
#endif
