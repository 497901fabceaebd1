/*
 * e2e_ctc.h -- C ABI of the MI355X-native CTC loss-and-decode library
 * (libe2e_ctc.so, built from end2end_amd/csrc/ with hipcc --offload-arch=gfx950).
 *
 * This is the drop-in boundary for the hot path of artbataev/end2end: every
 * entry point replaces one method of the reference's pybind11 engines
 * (citations are file:line in the reference tree).  Plain pointers and sizes
 * only; no torch / pybind types.  All data pointers are DEVICE pointers on the
 * current HIP device unless a parameter says "host".  Every call is
 * asynchronous on `stream` (a hipStream_t passed as void*; NULL = the null
 * stream), allocates nothing and never synchronises, so it can be captured in
 * a hipGraph; the caller owns every buffer.
 *
 * Return value: 0 on success, a negative E2E_ERR_* code otherwise;
 * e2e_last_error() then returns a thread-local message.  No C++ exception
 * crosses this boundary.
 */
#ifndef E2E_CTC_H
#define E2E_CTC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define E2E_CTC_ABI_VERSION 4

/* element types of the logits / log-prob tensor (losses and grads use the same) */
#define E2E_F32 0
#define E2E_F64 1
/* 16-bit inputs (e2e_ctc_loss_fwd_bwd(_opt) under E2E_ALGO_AUTO / E2E_ALGO_FAST, e2e_ctc_greedy): the logits are read in
 * their own dtype, the lattice runs in f32 (fast / wide path; reference: src/losses/forward_backward.cpp:15 converts once
 * to double), and the gradient is written in the source dtype.  `losses` and `reduced` are FLOAT32 for these two -- a
 * loss of a few hundred has three digits in bf16 --; the Python engine converts the B losses at the end.  Shapes the
 * fast and wide paths do not take return E2E_ERR_UNSUPPORTED for these dtypes (up-cast and call again). */
#define E2E_F16 2
#define E2E_BF16 3

#define E2E_OK 0
#define E2E_ERR_ARG (-1)          /* bad argument (null pointer, bad size/dtype) */
#define E2E_ERR_UNSUPPORTED (-2)  /* shape outside what the kernels support */
#define E2E_ERR_WORKSPACE (-3)    /* workspace too small */
#define E2E_ERR_HIP (-4)          /* a HIP launch / runtime call failed */
#define E2E_ERR_IO (-5)           /* LM file could not be read / parsed (host) */

/* which CTC loss algorithm to run */
#define E2E_ALGO_AUTO 0    /* fast scaled path for f32 where valid; otherwise the exact kernel -- for f32 in its rescaled
                            * f64 probability-domain form, for f64 in the reference's log domain */
#define E2E_ALGO_EXACT 1   /* f64 log-domain lattice, the reference's arithmetic */
#define E2E_ALGO_FAST 2    /* scaled linear-domain lattice, flags invalid utterances */

int e2e_ctc_abi_version(void);
const char* e2e_last_error(void);

/* ------------------------------------------------------------------------
 * CTC loss forward + backward.
 * Replaces cpp_ctc_loss.CTCLossEngine(blank_idx).compute(logits, targets,
 * logits_lengths, targets_lengths) -> (losses[B], grads[B,T,V])
 *   src/losses/ctc_loss_py.cpp:8-16, src/losses/forward_backward.cpp:7-59,
 *   src/losses/ctc_loss.cpp:15-118.
 *
 *   x            (B,T,V) tensor with element strides sB,sT,sV (a time-major
 *                permuted view is fine); dtype E2E_F32, E2E_F64, or -- where e2e_ctc_loss_takes_dtype() says so --
 *                E2E_F16 / E2E_BF16 (read as they are: no f32 copy exists)
 *   input_is_logprobs
 *                1: x holds log-probabilities -- exactly the reference engine:
 *                   grads = exp(x) - posterior over the full (T,V) slab, rows
 *                   t >= x_len[b] come out as exp(x) (reference quirk Q1);
 *                0: x holds raw logits; log_softmax(dim=V) is fused in and
 *                   grads are d loss / d logits (= softmax - posterior for
 *                   t < x_len[b], 0 for padded rows), i.e. what
 *                   pytorch_end2end/modules/ctc_loss.py:37-40 + autograd give.
 *   targets      (B,Smax) int64, row stride tgt_stride (>= Smax), first t_len[b] entries used; what lies beyond them is never read
 *   Smax         the WIDTH of the targets tensor.  It, not the longest target in the batch, selects the kernels (and sizes the
 *                workspace): a batch padded to 300 columns runs other kernels than the same batch at 200, with the same results
 *                (e2e_debug_loss_route in e2e_ctc_debug.h tells which).  A target is compared with [0,V) as the int64 it is.
 *   x_len,t_len  (B) int64 (1 <= x_len[b] <= T, 0 <= t_len[b] <= Smax).  An utterance whose lengths are
 *                outside these ranges, or whose first t_len[b] targets contain a value outside [0,V), gets
 *                loss = NaN and a NaN gradient slab (the reference reads out of bounds there); the other
 *                utterances of the batch are unaffected and the call still returns 0.
 *   losses       (B)  same dtype as x -- f32 for 16-bit x;  +inf for an infeasible alignment (Q2)
 *   grads        (B,T,V) contiguous, same dtype as x (16-bit x: 16-bit gradient); NaN slab when infeasible
 *   workspace    >= e2e_ctc_loss_workspace_bytes(...) bytes, 256-B aligned
 *   algo         E2E_ALGO_*
 */
size_t e2e_ctc_loss_workspace_bytes(int B, int T, int V, int Smax, int dtype, int algo);

/* 1 if a loss call with these logits runs as it is; 0 if the caller has to up-cast them to f32 first (then the call would
 * return E2E_ERR_UNSUPPORTED).  Always 1 for E2E_F32 / E2E_F64.  16-bit logits are read natively by the lattice kernels
 * (alphabets of <= 448 columns, targets of <= 447 labels: any strides) and by the wide-alphabet path -- in one pass when its rows
 * are contiguous (sV == 1), V % 8 == 0, V <= 8192, strides of whole 16-byte pieces, x and grads 16-byte aligned; element by
 * element in two passes otherwise (since ABI 3).  What is left for 0: shapes only the exact kernel takes (E2E_ALGO_EXACT, or
 * targets beyond 447 labels on an alphabet the wide path does not compact). */
int e2e_ctc_loss_takes_dtype(int dtype, int algo, int T, int V, int Smax, int64_t sB, int64_t sT, int64_t sV,
                             const void* x, const void* grads);

int e2e_ctc_loss_fwd_bwd(const void* x, int dtype, int input_is_logprobs,
                         int64_t sB, int64_t sT, int64_t sV,
                         const int64_t* targets, int64_t tgt_stride,
                         const int64_t* x_len, const int64_t* t_len,
                         int B, int T, int V, int Smax, int blank,
                         void* losses, void* grads,
                         void* workspace, size_t workspace_bytes,
                         int algo, void* stream);

/* The same call with options (NULL = the plain call):
 *   grad_scale  every gradient element is multiplied by it as it is written (NaN slabs stay NaN).  The module passes
 *               1/B for reduce=True, size_average=True, so that the autograd backward of the mean
 *               (pytorch_end2end/modules/ctc_loss.py:52-56 + functions/forward_backward.py:33) has nothing left to do.
 *   reduced     NULL, or one element of x's dtype that receives the sum (E2E_REDUCE_SUM) or mean (E2E_REDUCE_MEAN) of
 *               the B losses (+inf / NaN propagate as they would through torch.sum), in a fixed order (deterministic).
 *               On the f32 small-alphabet path it is written by the launch that also looks for flagged utterances, so
 *               the call has no launch more than without it.
 *   chains      arithmetic of the lattice chains on the f32 small-alphabet path.  E2E_CHAINS_F64 (0, the default): every
 *               result within ~1e-6 of the reference's f64 (gradient elements: 2e-6 absolute).  E2E_CHAINS_F32: the
 *               chains run in packed f32 where that is faster (targets longer than 127 labels: ~10 % on the step at
 *               B=256, T=1000, V=29, S<=200); losses still within 2e-6 relative, gradient elements within 2e-5 absolute -- inside the
 *               1e-4 the drop-in promises, for callers that train in f32 / bf16 anyway.  Elsewhere it changes nothing. */
#define E2E_REDUCE_NONE 0
#define E2E_REDUCE_SUM 1
#define E2E_REDUCE_MEAN 2
#define E2E_CHAINS_F64 0
#define E2E_CHAINS_F32 1
typedef struct e2e_ctc_loss_opts {
  double grad_scale;
  void* reduced;
  int reduction;
  int chains;
} e2e_ctc_loss_opts;

int e2e_ctc_loss_fwd_bwd_opt(const void* x, int dtype, int input_is_logprobs,
                             int64_t sB, int64_t sT, int64_t sV,
                             const int64_t* targets, int64_t tgt_stride,
                             const int64_t* x_len, const int64_t* t_len,
                             int B, int T, int V, int Smax, int blank,
                             void* losses, void* grads,
                             void* workspace, size_t workspace_bytes,
                             int algo, void* stream, const e2e_ctc_loss_opts* opts);

/* grads[b,:,:] *= scale[b]  in place (rows whose factor is exactly 1 are not touched): the multiply of the autograd backward
 * (pytorch_end2end/functions/forward_backward.py:33) without a second (B,T,V) tensor. */
int e2e_ctc_scale_grads(void* grads, int dtype, const void* scale /* (B) same dtype */,
                        int B, int64_t row_elems /* T*V */, void* stream);

/* ------------------------------------------------------------------------
 * CTC without blank (ASG-style) loss forward + backward (since ABI 4).
 * Replaces pytorch_end2end.functions.ctc_without_blank.CTCWithoutBlankLossFunction
 *   pytorch_end2end/functions/ctc_without_blank.py:13-138 (a numba lattice on host copies upstream).
 *   x            (B,T,V) tensor with element strides sB,sT,sV (any strides); dtype E2E_F32 or E2E_F64 only -- the Python
 *                engine up-casts 16-bit inputs to f32 before the call
 *   input_is_logprobs
 *                1: x holds log-probabilities -- upstream's function: grads = exp(x) - posterior on rows t < x_len[b];
 *                0: x holds raw logits; log_softmax(dim=V) is fused in and grads are d loss / d logits
 *                   (= softmax - posterior).
 *                Either way padded rows t >= x_len[b] are 0 (upstream fills only rows t < x_len, np.zeros_like).
 *   targets      (B,*) int64, row stride tgt_stride, first t_len[b] entries used
 *   space_idx    -1 (none) or a label in [0,V) wrapped around the target: ext = [sp] + target + [sp]; an empty target or
 *                the target [sp] gives ext = [space_idx].  Quirk Q10: space_idx = -1 with an empty target gives ext = [-1],
 *                which upstream's numpy indexing reads as column V-1 -- reproduced.  Anything else: E2E_ERR_ARG.
 *   lattice      from cell j a frame stays at j or moves to j+1 (no blank, no skip, repeats allowed); start cell 0
 *                (and 1 with spaces), end cell L'-1 (and L'-2 with spaces)
 *   x_len,t_len  (B) int64 (1 <= x_len[b] <= T, 0 <= t_len[b] <= Smax); lengths outside these ranges or a target outside
 *                [0,V) give loss = NaN and a NaN gradient slab for that utterance only
 *   losses       (B) same dtype as x (upstream always returns float32: a deliberate difference, as Q3, so that f64
 *                gradcheck works); +inf for an infeasible utterance, whose rows t < x_len[b] are then NaN (as Q2)
 *   grads        (B,T,V) contiguous, same dtype as x
 *   workspace    >= e2e_ctc_noblank_workspace_bytes(...) bytes: per-frame row statistics, alpha checkpoints every K
 *                frames (K below) and a per-utterance redo flag (B=256, T=1000, Smax=200: 29 MB)
 *   opts         NULL, or e2e_ctc_loss_opts: grad_scale and reduced / reduction as for e2e_ctc_loss_fwd_bwd_opt; `chains`
 *                is ignored
 * f32 inputs run a rescaled probability-domain lattice with f64 cells; an utterance it cannot settle is redone in the f64
 * log domain in the same call.  f64 inputs run the reference's log-domain arithmetic.  The lattice rows live in one
 * workgroup's LDS, in blocks of K frames, K the checkpoint interval: K = 16 up to Smax = 235, then fewer (15 from 236, 11
 * from 308, 8 from 399, 5 from 566, 3 from 784, 2 from 972, 1 from 1 276).  Targets of up to Smax = 1 855 labels; beyond
 * that E2E_ERR_UNSUPPORTED (workspace_bytes then returns 0).
 */
size_t e2e_ctc_noblank_workspace_bytes(int B, int T, int V, int Smax, int dtype);

int e2e_ctc_noblank_fwd_bwd(const void* x, int dtype, int input_is_logprobs, int64_t sB, int64_t sT, int64_t sV,
                            const int64_t* targets, int64_t tgt_stride, const int64_t* x_len, const int64_t* t_len,
                            int B, int T, int V, int Smax, int space_idx, void* losses, void* grads,
                            void* workspace, size_t workspace_bytes, void* stream, const e2e_ctc_loss_opts* opts);

/* ------------------------------------------------------------------------
 * Gram-CTC loss forward + backward (since ABI 4; Liu et al., ICML 2017, arXiv:1703.00096).
 * Replaces cpp_gram_ctc_loss.GramCTCLossEngine(blank_idx, num_base_labels, total_labels, label2ids).compute(...), whose
 *   compute_2d is empty upstream (src/losses/gram_ctc_loss.cpp:30-37).  The definition (upstream never fixed one):
 *   columns      0 the blank; c in [1, radix) the unigram (c); c in [radix, V) a gram, a sequence of 1..8 base labels
 *   labelling    of a path (one column per frame): collapse runs of one column, drop blanks, concatenate the grams'
 *                base sequences.  The loss is -log of the total probability of the paths whose labelling is the target.
 *                Two identical grams in a row need a blank between them; different grams do not.
 *   lattice      boundaries j = 0..S of the target: a blank state at each, a gram state (j, k) wherever y[j-k..j-1] is a
 *                gram (k <= max_order).  blank(j) <- itself, every gram state ending at j; gram(j, k) <- itself,
 *                blank(j-k), every gram state ending at j-k but one of the same column.  Start blank(0), gram(k, k); end
 *                blank(S), every gram(S, k).  With unigrams only (V = radix) this is CTC with blank 0.
 * Parameters as e2e_ctc_noblank_fwd_bwd, without space_idx, and:
 *   targets      (B,*) int64 base-label ids in [1, radix); a target outside that range, or x_len / t_len outside
 *                1 <= x_len[b] <= T, 0 <= t_len[b] <= Smax, gives loss = NaN and a NaN gradient slab for that utterance
 *   keys, cols   the gram table, device: n_grams int64 keys sorted ascending and the int32 column of each.  The key of a
 *                gram (y_1 .. y_k) is the polynomial y_1 * radix^(k-1) + ... + y_k (ids >= 1: keys of different orders
 *                never collide).  It holds every column in [1, V): the unigram c has the key c.  Keys must be distinct.
 *   n_grams      entries of the table (>= 0; keys / cols may be NULL when 0)
 *   radix        R = number of base labels, the blank counted: base ids are 1 .. R-1; 1 <= R <= V
 *   max_order    the longest gram, 1..8; radix ** max_order must fit in int64
 *   losses       (B) same dtype as x; +inf for an infeasible utterance (no path spells the target in x_len[b] frames, or
 *                every such path has probability 0), whose rows t < x_len[b] are then NaN
 *   grads        (B,T,V) contiguous, same dtype as x: softmax - posterior (input_is_logprobs = 0) or exp(x) - posterior
 *                (1) on rows t < x_len[b], 0 beyond
 *   workspace    >= e2e_gram_ctc_workspace_bytes(...) bytes: per-frame row statistics and alpha checkpoints every 16
 *                frames, B*T*8 + B*ceil(T/16)*((Smax+1)*(max_order+1)*8 + 4) + B*4 bytes (B=256, T=1000, Smax=200,
 *                max_order=3: 106 MB)
 *   opts         NULL, or e2e_ctc_loss_opts: grad_scale and reduced / reduction as for e2e_ctc_loss_fwd_bwd_opt; `chains`
 *                is ignored
 * f32 inputs run a rescaled probability-domain lattice with f64 cells; an utterance it cannot settle is redone in the f64
 * log domain in the same call.  f64 inputs run the log domain throughout.  The lattice rows live in one workgroup's LDS:
 * targets of up to Smax = 668 labels at max_order 3 (1 316 at 1, 887 at 2, 536 at 4, 299 at 8); beyond that the call
 * returns E2E_ERR_UNSUPPORTED and e2e_gram_ctc_workspace_bytes returns 0.
 */
size_t e2e_gram_ctc_workspace_bytes(int B, int T, int V, int Smax, int max_order, int dtype);

int e2e_gram_ctc_fwd_bwd(const void* x, int dtype, int input_is_logprobs, int64_t sB, int64_t sT, int64_t sV,
                         const int64_t* targets, int64_t tgt_stride, const int64_t* x_len, const int64_t* t_len,
                         int B, int T, int V, int Smax, const int64_t* keys, const int32_t* cols, int n_grams,
                         int radix, int max_order, void* losses, void* grads,
                         void* workspace, size_t workspace_bytes, void* stream, const e2e_ctc_loss_opts* opts);

/* ------------------------------------------------------------------------
 * ASG, the Auto Segmentation Criterion with learned transitions (additive, ABI 4; Collobert et al. 2016, arXiv:1609.03193).
 * Upstream names it (ASGEncoder raises NotImplementedError, pytorch_end2end/encoders/text_encoders.py) and has no loss.
 * The definition, with n = x_len[b], s = t_len[b], y = targets[b, :s]:
 *   path score   score(pi) = sum_{t<n} x[b,t,pi_t] + sum_{1<=t<n} A[pi_t, pi_{t-1}]; no start or end transition, and no
 *                softmax anywhere: x holds unnormalised scores
 *   FCC_b        log sum over all pi in {0..V-1}^n of exp(score(pi)): the fully connected graph
 *   FAL_b        log sum over the alignments k of exp(score(y_k(0) .. y_k(n-1))), k(0) = 0, k(n-1) = s-1,
 *                k(t) - k(t-1) in {0, 1}.  Alignments are counted by k, not by the labels they spell: with a repeated
 *                label (a a) the entry A[a,a] carries mass both as "stay" and as "advance"
 *   loss_b       FCC_b - FAL_b >= 0
 * e2e_asg_fwd_bwd:
 *   x            (B,T,V) emissions with element strides sB,sT,sV (any strides); E2E_F32 or E2E_F64 only -- the Python
 *                engine up-casts 16-bit inputs to f32 before the call
 *   transitions  (V,V) contiguous, x's dtype: A[j,i] (row = to, column = from: the wav2letter / flashlight layout) is
 *                the score of label j at frame t after label i at frame t-1.  Finite numbers; -inf is not supported
 *   targets      (B,*) int64, row stride tgt_stride, first t_len[b] entries used; what lies beyond them is never read
 *   x_len,t_len  (B) int64 (1 <= x_len[b] <= T, 1 <= t_len[b] <= Smax: an empty target has no ASG lattice).  Lengths
 *                outside these ranges or a target outside [0,V) give loss = NaN, a NaN gradient slab and a NaN tgrads
 *                slab for that utterance only
 *   losses       (B) x's dtype; +inf for an infeasible utterance (x_len[b] < t_len[b]), whose rows t < x_len[b] of grads
 *                and whose tgrads slab are then NaN
 *   grads        (B,T,V) contiguous, x's dtype: grad_scale * (P_fcc(pi_t = v) - P_fal(pi_t = v)) on rows t < x_len[b],
 *                0 beyond
 *   tgrads       (B,V,V) contiguous, x's dtype: per utterance grad_scale * sum_{1<=t<n} (P_fcc(pi_t = j, pi_{t-1} = i)
 *                - P_fal(the same)); the parameter's gradient is the caller's sum_b w_b tgrads[b]
 *   workspace    >= e2e_asg_workspace_bytes(...) bytes: log alpha of both recurrences and the pair sums in f64,
 *                8 * (B*T*V + B*V*V + B + B*T*max(Smax,1)) bytes and alignment (B=256, T=1000, V=29, Smax=200: 471 MB;
 *                B=64, T=256, V=128, Smax=60: 33 MB)
 *   opts         NULL, or e2e_ctc_loss_opts: grad_scale multiplies both gradients; a reduction other than
 *                E2E_REDUCE_NONE returns E2E_ERR_UNSUPPORTED (sum the B losses); `chains` is ignored
 * All cells are f64 for both dtypes; the dense recurrence shifts every step by its row maximum, so there is no redo
 * route and nothing to read back.  Results are bit-identical from call to call and stream to stream (no atomics).
 * Limits (e2e_asg_max_labels, e2e_asg_max_target_length): 1 <= V <= 128 -- exp(A) lives in one workgroup's LDS, 132 KB of
 * 160 at V = 128 -- and Smax <= 512; every T.  Beyond them the call returns E2E_ERR_UNSUPPORTED and the workspace
 * queries return 0.
 *
 * e2e_asg_viterbi, the best path: delta_0[j] = x[0,j]; delta_t[j] = (max_i (delta_{t-1}[i] + A[j,i])) + x[t,j], evaluated
 * in f64 in exactly this order (f32 inputs convert exactly).  Ties go to the lowest i; the end state is the lowest j of the
 * largest delta_{n-1}.
 *   x, transitions, x_len   as above (no targets)
 *   path         (B,T) int64: the label of every frame t < x_len[b], pad_value beyond
 *   scores       (B) f64: the path's score (for every dtype of x)
 *   collapsed    (B,T) int64: the path with consecutive repeats merged, zero filled on the right; lengths (B) int64
 *   workspace    >= e2e_asg_viterbi_workspace_bytes(...) bytes: one-byte back-pointers, B*T*V bytes
 * An utterance with x_len[b] outside [1,T] gets a path of pad_value, score NaN and length 0.
 */
int e2e_asg_max_labels(void);
int e2e_asg_max_target_length(void);
size_t e2e_asg_workspace_bytes(int B, int T, int V, int Smax, int dtype);

int e2e_asg_fwd_bwd(const void* x, int dtype, int64_t sB, int64_t sT, int64_t sV, const void* transitions,
                    const int64_t* targets, int64_t tgt_stride, const int64_t* x_len, const int64_t* t_len,
                    int B, int T, int V, int Smax, void* losses, void* grads, void* tgrads, void* workspace,
                    size_t workspace_bytes, void* stream, const e2e_ctc_loss_opts* opts);

size_t e2e_asg_viterbi_workspace_bytes(int B, int T, int V);

int e2e_asg_viterbi(const void* x, int dtype, int64_t sB, int64_t sT, int64_t sV, const void* transitions,
                    const int64_t* x_len, int B, int T, int V, int64_t* path, int64_t pad_value, double* scores,
                    int64_t* collapsed, int64_t* lengths, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Gram-CTC decoding: greedy, and prefix beam search read out as an n-best list (additive, ABI 4: nothing above changes
 * meaning).  Columns and labelling are e2e_gram_ctc_fwd_bwd's: column 0 the blank, 1 .. R-1 the unigrams, R .. V-1 grams of
 * 1..8 base ids; a path is labelled by collapsing runs of one column, dropping blanks and concatenating the grams' base
 * sequences.  The decoders take the table spelled out, not as keys:
 *   gram_ids   (V,8) int32, device: the base ids of every column, zero padded (row 0, the blank's, is not read)
 *   gram_len   (V) int32, device: how many of them count, 1 .. max_order (entry 0 is not read; a value outside the range
 *              is clamped into it: the host cannot see the table)
 *   max_order  the longest gram, 1..8 (E2E_ERR_ARG otherwise)
 *
 * GREEDY.  Arg-max column per frame (ties as e2e_ctc_greedy breaks them: first maximum, NaN counts as the maximum),
 * collapse runs, drop the blank -- e2e_ctc_greedy with blank = 0 -- then every column expanded to its base ids.
 *   x          (B,T,V) logits or log-probs, strides sB,sT,sV; the four dtypes of e2e_ctc_greedy
 *   out        (B, T*max_order) int64 base ids, zero padded on the right; out_len (B) int64
 *   cols       (B,T) int64: the collapsed columns, zero padded -- the gram segmentation the model chose; cols_len (B).
 *              Both are required: the expansion reads them.
 *
 * BEAM SEARCH.  A hypothesis is a base-id prefix l with up to max_order + 1 SLOTS: slot 0 the mass of the paths that end in
 * the blank, slot k >= 1 the mass of the paths whose last column is the order-k gram that spells the last k ids of l, and
 * that column (gram keys are distinct: there is at most one).  Before frame 0 the beam is the empty prefix with mass 1 in
 * slot 0.  At frame t, with y = exp(lp[t]) and tot(l) the sum of l's slots:
 *   stay, blank           new[l].slot0 += tot(l) * y[0]
 *   stay, run continues   for every filled slot k >= 1 with column c: new[l].slotk += p_k(l) * y[c]
 *   extend                for every column c' >= 1 of order k': src = the sum of l's slots except a slot k' that holds c';
 *                         if src > 0 (and src * y[c'] > 0): new[l + gram(c')].slot k' += src * y[c'], its column c'
 * Candidates that spell the same base sequence are ONE hypothesis, whichever prefixes and columns they came from.  The new
 * beam is the beam_width hypotheses of largest tot.  A prefix that left the beam and is formed again starts from its
 * extension shares alone.
 *   identity   a prefix is its 64-bit key: key(empty) = 0xcbf29ce484222325, key(l + [i]) = (key(l) XOR i) * 0x100000001b3
 *              mod 2^64.  Two different prefixes with equal keys are merged: about 2^-64 per pair, i.e. correct with
 *              overwhelming probability, not by construction (as for the language-model tables above).  A key of 0 is
 *              kept as 1.
 *   ranking    everywhere -- the per-frame cut and the n-best list -- by tot descending and, for exactly equal values, by
 *              key ascending.  A (prefix, slot) receives at most two addends, its stay share and one extension share, and
 *              tot is the sum of the slots in the order 0 .. max_order: no result depends on the order in which the
 *              hardware meets the candidates, and two calls on the same input agree bit for bit.
 *   arithmetic f64 in the probability domain.  After each frame's cut every kept mass is divided by 2^e, e the binary
 *              exponent of the best hypothesis' tot (exact), and the e are summed into the score.  Mass that reaches
 *              exactly 0 is "not a member": a search in which underflow to 0 decides membership (probabilities some 300
 *              decades below the frame's best) is outside what is promised to equal the rules above.
 *   lp         (B,T,V) LOG-PROBABILITIES, strides sB,sT,sV, f32 or f64 (16-bit: up-cast first; E2E_ERR_ARG)
 *   x_len      (B) int64, clamped to 0..T; 0 yields the empty hypothesis alone, with score 0
 *   nbest      1 <= nbest <= beam_width, else E2E_ERR_ARG
 *   out        (B,nbest,max_out) int64 base ids, zero filled behind each hypothesis.  The empty hypothesis has length 0;
 *              there is no -1 id.  max_out = T * max_order can never be exceeded.
 *   out_len    (B,nbest) int64: 0 for slots >= n_hyp[b]; > max_out = truncated, that many ids were needed and the first
 *              max_out were written (as in e2e_ctc_beam_nbest)
 *   n_hyp      (B) int64: min(nbest, members of the final beam) -- below nbest when fewer sequences have non-zero
 *              probability; -1 = the candidate table or node pool ran out (cannot happen with a workspace of
 *              e2e_gram_beam_workspace_bytes(); nothing of the utterance may be used)
 *   scores     (B,nbest) f64: log tot, natural log; -inf in empty slots
 *   workspace  >= e2e_gram_beam_workspace_bytes(...): per utterance the frame's probabilities, an open-addressing table
 *              of 2 * beam_width * V keys rounded up to a power of two (16 bytes each), 28 bytes per (member, column)
 *              pair and 8 bytes per node of the pool of beam_width * (T + 1) + 1 (parent, column) nodes
 *              (B=64, T=1000, V=379, beam_width=100: 254 MB)
 * Limits: beam_width <= e2e_gram_beam_max_width(V, max_order) = min(128, 131072 / V) -- 128 up to V = 1024, 100 fits the
 * loss's headline table V = 379, 16 at V = 8000 --, T <= 2^22; beyond them E2E_ERR_UNSUPPORTED, found on the host before
 * any launch (e2e_gram_beam_workspace_bytes then returns 0).  The call is asynchronous on `stream`, allocates nothing,
 * never synchronises and is capturable.  With a word language model: e2e_gram_ctc_beam_nbest_lm, below; restricted to
 * a vocabulary, and with label timestamps: e2e_gram_ctc_beam_nbest_opt, below that; both fed in chunks:
 * e2e_gram_ctc_beam_stream, below that.  Not provided for Gram-CTC: custom
 * transcriptions, a word list together with a language model, a column
 * segmentation per beam hypothesis (several exist), blank_idx != 0.
 */
int e2e_gram_ctc_greedy(const void* x, int dtype, int64_t sB, int64_t sT, int64_t sV, const int64_t* x_len,
                        int B, int T, int V, const int32_t* gram_ids, const int32_t* gram_len, int max_order,
                        int64_t* out, int64_t* out_len, int64_t* cols, int64_t* cols_len, void* stream);

int e2e_gram_beam_max_width(int V, int max_order);
size_t e2e_gram_beam_workspace_bytes(int B, int T, int V, int max_order, int beam_width);

int e2e_gram_ctc_beam_nbest(const void* lp, int dtype, int64_t sB, int64_t sT, int64_t sV, const int64_t* x_len,
                            int B, int T, int V, const int32_t* gram_ids, const int32_t* gram_len, int max_order,
                            int beam_width, int nbest, int64_t* out, int64_t max_out, int64_t* out_len, int64_t* n_hyp,
                            double* scores, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Gram-CTC beam search with a word language model (additive, ABI 4: nothing above changes meaning).  The search, its slots,
 * its stay and extend rules, the key and the per-frame power-of-two rescale are e2e_gram_ctc_beam_nbest's, unchanged; a
 * hypothesis is still a base-id sequence, whichever columns spelled it.  What changes is what the cut and the ranking compare.
 *   LM fields    lm_score, num_words, num_oov and the LM state are functions of the base-id sequence alone: e2e_ctc_beam's
 *                rules (as e2e_asg_beam_nbest states them) applied to the base ids one at a time, as if each had been appended
 *                on its own.  A word starts at a non-space id after the empty prefix or after the space; at every non-space id
 *                the model is asked with the partial word as if it were complete: lm_score = lm_before +
 *                base_score(state_before, idx(word)) / ln 10, num_oov = oov_before + (idx == 0); a space copies the fields;
 *                case folding and byte comparison as in e2e_ctc_beam.  An extension by a gram of k ids applies the rule k
 *                times (a gram may hold the space: it can end one word and begin the next).  Only the queries at a word's
 *                last id inside the gram and at the gram's last id can influence the result; the others may be skipped,
 *                the result is the same bits.  A hypothesis reached from several (parent, column) pairs has identical
 *                fields from each -- same bits, same chain of additions: no result depends on which pair is used
 *   totals, cut  for the frame's cut and for the final ranking a candidate's total is
 *                log(tot) + lmwt * lm_score - wip * num_words + oov_penalty * num_oov, evaluated left to right, tot the
 *                candidate's mass in the frame's scaling (without the common exponent sum).  A candidate with tot <= 0, or
 *                with a NaN or -inf total, is no candidate.  The beam_width largest totals are kept, exactly equal totals
 *                by key ascending.  The rescale uses the rank-0 survivor's tot.  The n-best list is in the last cut's order
 *   space_id     the space's base id, or negative: none -- the whole sequence is then one word (>= num_base_labels:
 *                E2E_ERR_ARG)
 *   lm           NULL or a model of e2e_lm_load_arpa on the current device, loaded with exactly num_base_labels label
 *                strings (index 0, the blank's, is never spelled; gram columns have no strings of their own); order <= 6.
 *                NULL: lmwt counts as 0, wip still applies (num_words needs only space_id).  A model with custom
 *                transcriptions (e2e_lm_load_transcriptions) or one that is only a word list (e2e_lm_load_words) is
 *                refused with E2E_ERR_ARG
 *   scores       (B,nbest,3) f64: total, ac, lm_score.  ac = log tot + e ln 2 is e2e_gram_ctc_beam_nbest's score, total the
 *                formula above with ac in place of log(tot).  Slots >= n_hyp[b]: -inf, -inf, 0
 *   counts       (B,nbest,2) int32: num_words, num_oov -- the layout of e2e_asg_beam_nbest
 *   x_len[b] = 0 gives the empty hypothesis with all scores 0 and both counts 0
 *   workspace    >= e2e_gram_beam_workspace_bytes_lm(..., with_lm): with_lm = 0 is e2e_gram_beam_workspace_bytes, and serves
 *                a call with lm == NULL as well; with_lm = 1 adds, per utterance, the children's answers of 2 * beam_width
 *                prefixes: 16 bytes per (prefix, column) (B=64, T=1000, V=379, beam_width=100: + 78 MB)
 * Everything else -- lp, x_len, the table, nbest, out, out_len, n_hyp, the limits (e2e_gram_beam_max_width) -- is
 * e2e_gram_ctc_beam_nbest's.  Every argument error is found on the host before any launch.  Asynchronous on `stream`,
 * allocates nothing, never synchronises, capturable.  Two calls on the same input agree bit for bit.
 */
struct e2e_lm;   /* (e2e_lm_load_arpa, below) */
size_t e2e_gram_beam_workspace_bytes_lm(int B, int T, int V, int max_order, int beam_width, int with_lm);

int e2e_gram_ctc_beam_nbest_lm(const void* lp, int dtype, int64_t sB, int64_t sT, int64_t sV, const int64_t* x_len,
                               int B, int T, int V, const int32_t* gram_ids, const int32_t* gram_len, int max_order,
                               int num_base_labels, int beam_width, int space_id, const struct e2e_lm* lm, double lmwt,
                               double wip, double oov_penalty, int nbest, int64_t* out, int64_t max_out, int64_t* out_len,
                               int64_t* n_hyp, double* scores, int32_t* counts, void* workspace, size_t workspace_bytes,
                               void* stream);

/* ------------------------------------------------------------------------
 * Gram-CTC beam search restricted to a vocabulary, and label timestamps (additive, ABI 4: nothing above changes meaning).
 *
 * e2e_gram_ctc_beam_nbest_opt is e2e_gram_ctc_beam_nbest_lm with options; opts == NULL, or both fields zero, is
 * e2e_gram_ctc_beam_nbest_lm bit for bit.  The workspace (e2e_gram_beam_workspace_bytes_lm) and the width limits do not change.
 *
 * restrict_to_lexicon   L and Pref(L) are those of e2e_ctc_beam_nbest_opt: the model's words, folded as the lookup folds them,
 *                       and every non-empty byte prefix of a word.  A hypothesis is a base-id sequence, as before; its LAST WORD
 *                       is the run of ids after its last space, spelled as the LM lookup of e2e_gram_ctc_beam_nbest_lm spells it.
 *                       A step y -> y + (i) by one base id i obeys the rule if
 *                         - i is not the space and the last word of y + (i) is spelled in Pref(L); or
 *                         - i is the space and y is empty, ends in the space, or ends in a word of L (e2e_ctc_beam_nbest_opt's
 *                           space rule, not ASG's: base-id sequences can repeat an id, so a space can follow a space).
 *                       A sequence is ADMISSIBLE if every one of its base-id prefixes obeys the rule; an extension by a gram of k
 *                       ids applies the rule k times.  Admissibility is a function of the sequence alone, not of the columns
 *                       that spelled it: `a`,`b` and the gram `ab` agree.  A restricted search forms only admissible sequences:
 *                       a (member, column) pair whose extension is inadmissible gives nothing and creates no candidate.  Slots,
 *                       stay shares, keys, the rescale, LM fields, totals, the cut, tie order and the read-out are
 *                       e2e_gram_ctc_beam_nbest_lm's.  The last word of a result may be a proper prefix that is no word: it
 *                       counts as out of vocabulary, as it always did.  If no first label is admissible and the blank has no
 *                       mass, no hypothesis is left: n_hyp[b] = 0.
 *                       Pref(L) is prefix-closed, so the rule is decided where the model is asked anyway: a word that ends
 *                       before a space inside the gram must be a word of L; the spelling at the gram's last id, if that is no
 *                       space, must be in Pref(L); a gram that begins with the space needs the parent's last word to be a word
 *                       of L (its last lookup counted no OOV).
 *                       != 0 with lm == NULL or a model without a lexicon (e2e_lm_enable_lexicon): E2E_ERR_ARG, before any
 *                       launch.  A transcription model stays refused (E2E_ERR_ARG).  A word-list model (e2e_lm_load_words) is
 *                       accepted by this entry, and only together with restrict_to_lexicon; e2e_gram_ctc_beam_nbest_lm keeps
 *                       refusing it.
 * timesteps             NULL, or (B,nbest,max_out) int64: for every id written to `out`, the creation frame of the pool node
 *                       that carries it, (node - 1) / beam_width, read during the read-out's backward walk: no workspace, no
 *                       per-frame work.  All ids of one gram column share a frame.  Values lie in [0, x_len[b]) and never
 *                       decrease along a sequence; from one node to the next they increase strictly.  Behind a sequence, and in
 *                       slots >= n_hyp[b]: -1; x_len[b] = 0 gives -1 throughout.  The first value need not be 0: the empty
 *                       prefix is a member and may stay.  A member that stays keeps its node.  A new sequence's node records the
 *                       pair with the least m * V + c among the (member at beam position m, column c) pairs that gave it a
 *                       non-zero share in that frame, and through it the parent's node: this is what makes the earlier labels'
 *                       frames well defined when several pairs spell one sequence.
 *                       The caveat of e2e_ctc_beam_nbest's timesteps holds here too: in a wide beam a sequence can enter the
 *                       beam before its last label becomes likely, so a value can precede the frame where the label is heard.
 * Asynchronous on `stream`, allocates nothing, never synchronises, capturable.
 */
typedef struct e2e_gram_beam_opts {
  int restrict_to_lexicon;   /* 0: the plain search */
  int64_t* timesteps;        /* NULL, or (B,nbest,max_out) int64 */
} e2e_gram_beam_opts;

int e2e_gram_ctc_beam_nbest_opt(const void* lp, int dtype, int64_t sB, int64_t sT, int64_t sV, const int64_t* x_len,
                                int B, int T, int V, const int32_t* gram_ids, const int32_t* gram_len, int max_order,
                                int num_base_labels, int beam_width, int space_id, const struct e2e_lm* lm, double lmwt,
                                double wip, double oov_penalty, int nbest, int64_t* out, int64_t max_out, int64_t* out_len,
                                int64_t* n_hyp, double* scores, int32_t* counts, void* workspace, size_t workspace_bytes,
                                void* stream, const e2e_gram_beam_opts* opts);

/* ------------------------------------------------------------------------
 * Streaming Gram-CTC beam search: e2e_gram_ctc_beam_nbest / e2e_gram_ctc_beam_nbest_opt fed in chunks, the beam kept on the
 * device between the calls (additive, ABI 4: nothing above changes meaning).  The conventions are e2e_asg_beam_stream's and
 * e2e_ctc_beam_stream's.
 *
 *   scored       0: the search and the outputs of e2e_gram_ctc_beam_nbest -- the cut on the bits of the masses, scores
 *                (B,nbest); lm, counts and opts must be NULL (E2E_ERR_ARG), num_base_labels, space_id and the knobs are not read.
 *                != 0: e2e_gram_ctc_beam_nbest_opt -- the cut on the totals' order keys, scores (B,nbest,3), counts (B,nbest,2),
 *                lm NULL or a model, opts NULL or restrict_to_lexicon / timesteps.  The two searches need not break ties
 *                alike (the bits of tot against the bits of log tot), so neither stands in for the other.
 * An utterance's search lives in one STATE ROW of device memory that the caller owns.  Its parts, each rounded up to 256
 * bytes: a 256-byte header, the beam's current members as they stand in the kernel's LDS (slot masses, slot columns, key,
 * tot, node, length: 16896 bytes), with `scored` their language-model fields (11776 bytes), and the pool of
 * beam_width * (max_frames + 1) + 1 (parent, column) nodes of 8 bytes.  The header holds 4-byte fields in this order: a magic
 * value; the configuration V, max_order, num_base_labels (0 unless scored), beam_width, scored, model or not, restricted or not,
 * max_frames; the member count, the frames consumed, the sticky overflow flag (byte 44), whether the beam is dead; and at byte
 * 56 the 8-byte sum of the exponents taken out so far.  A call resumes every utterance from its row, runs chunk_len[b] further
 * frames, stores the row and reads the current beam out.  What a frame rebuilds anyway is not stored: the candidate table is
 * empty between frames, the pair buffers are a frame's scratch, and the cache of the children's answers is recomputed at
 * resume -- the resumed members take its rows 0 .. n - 1 and their children's answers are computed as the per-frame refill
 * computes a new member's; they are functions of the sequence alone, so no output bit depends on the row a member holds.
 * A node's index, 1 + frame * beam_width + rank, counts the frames of the STREAM, so the timesteps need no storage.
 *   - A row whose first 256 bytes are zero is a fresh utterance: hipMemsetAsync (or zeroing the header) opens or resets a
 *     stream, no other call is needed.  The rest of a fresh row may hold anything.
 *   - Rows are self-contained: indices, no addresses.  They may be moved, permuted, gathered or reordered between calls,
 *     and a batch may mix fresh rows with rows of any age.
 *   - The call is asynchronous on `stream`, allocates nothing, does not synchronise and is capturable.
 *   - Every argument error the host can see is found before any launch, with the whole calls' codes; in addition nbest
 *     outside [0, beam_width], max_frames outside [1, 2^22], row_bytes below the query or no multiple of 8, and scored = 0
 *     together with a model, counts or opts (all E2E_ERR_ARG).
 * CONTRACT.  After chunks whose lengths for utterance b sum to f_b >= 0 -- fed with the same table, beam_width, model, lmwt /
 * wip / oov_penalty and options throughout -- every output of the read-out (out, out_len, n_hyp, scores, counts,
 * opts->timesteps) equals, bit for bit, what the whole call writes for the concatenated frames with x_len[b] = f_b and the
 * same nbest, max_out and options.  f_b = 0 is the whole call's utterance of length 0: a fresh row read out before any frame
 * gives the one empty hypothesis with acoustic score 0.  Timesteps are frames of the stream, not of the chunk.  A beam that
 * died (n_hyp = 0) stays dead over later chunks; a stream whose candidate table ran out reads out n_hyp = -1 from then on.
 *   lp           (B,T,V) log-probabilities of this chunk, strides sB,sT,sV, E2E_F32 or E2E_F64 (chunks may differ in dtype)
 *   chunk_len    (B) int64, device: frames of this chunk per utterance, clamped to 0..T.  0 runs no frame and stores
 *                nothing: the read-out repeats the utterance's last result
 *   state        (B,row_bytes) device, 8-byte aligned; row_bytes >= e2e_gram_beam_stream_row_bytes(...), a multiple of 8
 *   max_frames   the longest stream a row can hold, 1 .. 2^22; part of the row's configuration, checked at resume
 *   nbest        0: feed only, no read-out: the outputs up to counts (and opts->timesteps) may be NULL and are not touched;
 *                else 1 .. beam_width
 *   frames_done  (B) int64, device.  What only the device knows is reported here per utterance, and mirrored in n_hyp[b]
 *                when nbest > 0:
 *                  >= 0  frames consumed so far
 *                  -2    this chunk would pass max_frames
 *                  -3    the row was not written under this configuration
 *                Both statuses are found before anything of the row is touched: they leave the whole row byte for byte and
 *                write none of the utterance's other outputs, and the other utterances advance.
 *   workspace    >= e2e_gram_beam_stream_workspace_bytes(...): the whole call's per utterance without the node pool, which
 *                is the row's; it does not depend on the frames
 *   opts         NULL or e2e_gram_beam_opts (scored only); restrict_to_lexicon the same for every chunk, timesteps NULL or
 *                (B,nbest,max_out) per call
 * Row size: 256 + 16896 + (11776 scored) + 8 * (beam_width * (max_frames + 1) + 1) rounded up to 256, whatever the alphabet
 * and with or without a model; 0 for a width, alphabet or max_frames that is not supported, and for with_lm without scored.
 * beam_width 100, max_frames 30 000: 24 029 952 bytes scored, 24 MB per utterance, the node pool being all but 29 KB of it.
 */
size_t e2e_gram_beam_stream_row_bytes(int max_frames, int V, int max_order, int beam_width, int scored, int with_lm);
size_t e2e_gram_beam_stream_workspace_bytes(int B, int V, int max_order, int beam_width, int scored, int with_lm);

int e2e_gram_ctc_beam_stream(const void* lp, int dtype, int64_t sB, int64_t sT, int64_t sV, const int64_t* chunk_len,
                             int B, int T, int V, const int32_t* gram_ids, const int32_t* gram_len, int max_order,
                             int num_base_labels, int beam_width, int scored, int space_id, const struct e2e_lm* lm, double lmwt,
                             double wip, double oov_penalty, void* state, size_t row_bytes, int max_frames,
                             int nbest, int64_t* out, int64_t max_out, int64_t* out_len, int64_t* n_hyp, double* scores,
                             int32_t* counts, int64_t* frames_done, void* workspace, size_t workspace_bytes, void* stream,
                             const e2e_gram_beam_opts* opts);

/* ------------------------------------------------------------------------
 * Gram-CTC beam search with per-frame label pruning (cutoff_top_n, cutoff_prob) -- additive, ABI 4; the knobs and the
 * selection are e2e_ctc_label_cut's, defined with the CTC search's pruning further down.
 *
 * DEFINITION.  A frame's kept set is exactly steps 1 to 5 of e2e_ctc_label_cut with blank = 0 over the V columns of the row
 * the search reads (f32 and f64 as they are; 16-bit inputs are up-cast first, as for the unpruned calls).  Grams are columns
 * like any other.  In the search a column outside the frame's set does nothing in that frame:
 *   - it gives no extension share, from any member;
 *   - a slot that holds it receives no "run continues" stay share.
 * The blank's stay share is always there.  Everything else is unchanged: identity by key, the ranking, the two-addend slots,
 * the power-of-two rescale, the LM fields, the restriction rule, the node numbering 1 + t * beam_width + rank and with it
 * the timesteps.
 * CONSEQUENCE.  A pruned call equals, bit for bit in every output (ids, lengths, n_hyp, scores, counts, timesteps), the
 * unpruned call on log-probabilities whose non-kept columns are replaced by -inf: an absent addend and an addend of exactly 0
 * give the same f64 sum, a pair whose share is 0 is no candidate and a total of 0 is no member in the unpruned search either.
 * cutoff_top_n >= V together with cutoff_prob == 1 is no pruning: the *_cut entries then are the unpruned entries -- the
 * same kernel, the same workspace query.
 *
 * e2e_gram_ctc_beam_nbest_cut: with scored = 0 the search and the outputs of e2e_gram_ctc_beam_nbest (lm, counts and opts
 * NULL, num_base_labels / space_id / lmwt / wip / oov_penalty not read, scores (B,nbest)); else those of
 * e2e_gram_ctc_beam_nbest_opt, opts included.  e2e_gram_ctc_beam_stream_cut: e2e_gram_ctc_beam_stream plus the knobs.  The
 * selection and the search run on `stream` in one call.  Nothing of a frame's work scales with V: with K = min(cutoff_top_n,
 * V) a member has K + 1 (member, column) pairs, so
 *   width      beam_width <= e2e_gram_beam_cut_max_width(V, max_order, cutoff_top_n) = min(128, 131072 / (K + 1)): 128 for
 *              every alphabet up to K = 1023
 *   workspace  >= e2e_gram_beam_cut_workspace_bytes(...) (a stream: e2e_gram_beam_cut_stream_workspace_bytes, T the chunk's):
 *              the frames' lists, (B,T,K+1) and (B,T) int32, and per utterance e2e_gram_ctc_beam_nbest's buffers with K + 1
 *              in V's place.  No answer rows of a language model: a pair's answer is computed in the frame.  A query returns
 *              0 where the call would be refused
 *   a stream   the knobs are the same for every chunk (the caller's contract, as for opts); the selection runs on each
 *              chunk; the state row's layout is e2e_gram_beam_stream_row_bytes', which e2e_gram_beam_cut_stream_row_bytes
 *              also answers beyond the unpruned width limit; after any chunking the read-out equals the whole pruned call,
 *              bit for bit
 * Argument errors are found on the host before any launch: cutoff_top_n < 1 and cutoff_prob outside (0, 1] are E2E_ERR_ARG,
 * K > e2e_ctc_label_cut_max() and a width above the limit E2E_ERR_UNSUPPORTED; everything else as for the unpruned entries
 * (a workspace that is too small: E2E_ERR_WORKSPACE).  Asynchronous on `stream`, allocates nothing, never synchronises.
 */
int e2e_gram_beam_cut_max_width(int V, int max_order, int cutoff_top_n);
size_t e2e_gram_beam_cut_workspace_bytes(int B, int T, int V, int max_order, int beam_width, int scored, int with_lm,
                                         int cutoff_top_n);
size_t e2e_gram_beam_cut_stream_workspace_bytes(int B, int T, int V, int max_order, int beam_width, int scored, int with_lm,
                                                int cutoff_top_n);
size_t e2e_gram_beam_cut_stream_row_bytes(int max_frames, int V, int max_order, int beam_width, int scored, int with_lm,
                                          int cutoff_top_n);

int e2e_gram_ctc_beam_nbest_cut(const void* lp, int dtype, int64_t sB, int64_t sT, int64_t sV, const int64_t* x_len,
                                int B, int T, int V, const int32_t* gram_ids, const int32_t* gram_len, int max_order,
                                int num_base_labels, int beam_width, int scored, int space_id, const struct e2e_lm* lm, double lmwt,
                                double wip, double oov_penalty, int nbest, int64_t* out, int64_t max_out, int64_t* out_len,
                                int64_t* n_hyp, double* scores, int32_t* counts, void* workspace, size_t workspace_bytes,
                                void* stream, const e2e_gram_beam_opts* opts, int cutoff_top_n, double cutoff_prob);

int e2e_gram_ctc_beam_stream_cut(const void* lp, int dtype, int64_t sB, int64_t sT, int64_t sV, const int64_t* chunk_len,
                                 int B, int T, int V, const int32_t* gram_ids, const int32_t* gram_len, int max_order,
                                 int num_base_labels, int beam_width, int scored, int space_id, const struct e2e_lm* lm, double lmwt,
                                 double wip, double oov_penalty, void* state, size_t row_bytes, int max_frames,
                                 int nbest, int64_t* out, int64_t max_out, int64_t* out_len, int64_t* n_hyp, double* scores,
                                 int32_t* counts, int64_t* frames_done, void* workspace, size_t workspace_bytes, void* stream,
                                 const e2e_gram_beam_opts* opts, int cutoff_top_n, double cutoff_prob);

/* ------------------------------------------------------------------------
 * ASG decoding: n-best prefix beam search with transitions and a word language model (additive, ABI 4: nothing above
 * changes meaning).  Upstream has no ASG decoder; this is the definition.  Path score, x, transitions A[to, from], V, x_len
 * and strides are e2e_asg_fwd_bwd's / e2e_asg_viterbi's: no softmax, no start or end transition.
 *   labelling    a path is labelled by merging consecutive equal labels.  A hypothesis is such a label sequence y: non-empty,
 *                no two equal neighbours.  ac(y) = log sum exp(score(pi)) over the paths pi of x_len[b] frames labelled y
 *   repeat labels  the last R = num_replabels columns (ASGEncoder's ids).  A sequence is SPELLABLE if no repeat label is
 *                its first label, directly follows the space label or directly follows another repeat label.  Unspellable
 *                sequences are not hypotheses: their paths belong to nothing.  R = 0: every sequence is spellable
 *   the search   the beam after frame t-1 holds at most beam_width members (y, a = last label, s = log mass).
 *                frame 0: candidate (c) with mass x[0,c] for every label c that may start a sequence;
 *                frame t >= 1, stay: every member puts (s + A[a,a]) + x[t,a] on its own sequence;
 *                frame t >= 1, extension: for every c != a for which y + (c) is spellable, (s + A[c,a]) + x[t,c] on y + (c).
 *                A candidate's mass is the log-sum of what it received -- at most its own stay and one extension from its
 *                parent, if the parent is a member: hi + log1p(exp(lo - hi)), symmetric in the two.  A sequence that is not
 *                a member has no mass; one that left the beam and is formed again starts from its extension share alone
 *   arithmetic   every cell f64 in the log domain for both dtypes (f32 converts exactly); a candidate whose total is -inf
 *                or NaN is no candidate.  -inf transitions are not supported
 *   LM fields    lm_score, num_words, num_oov and the LM state are functions of the sequence alone, by e2e_ctc_beam's rules:
 *                a word starts at a non-space label after the root or after a space; the model is asked at every label with
 *                the partial word as if it were complete: lm_score = lm_before + base_score(state_before, idx(word)) / ln 10,
 *                num_oov = oov_before + (idx == 0); a space copies the fields; without a model lmwt counts as 0 and wip
 *                still applies.  A word is spelled with its repeat labels EXPANDED: repeat label r appends the bytes of the
 *                character before it r more times (h e l <1> o looks up hello); case folding and byte comparison as in
 *                e2e_ctc_beam.  The model must have been loaded with V labels; the repeat columns' strings are not read
 *   identity     a sequence is its 64-bit key, e2e_gram_ctc_beam_nbest's: key(empty) = 0xcbf29ce484222325,
 *                key(y + (c)) = (key(y) XOR c) * 0x100000001b3 mod 2^64, 0 kept as 1; equal keys are one sequence (2^-64)
 *   cut, ranking total = ac + lmwt * lm_score - wip * num_words + oov_penalty * num_oov (evaluated left to right).  The
 *                beam_width largest totals are kept, ties by key ascending; the n-best list is in the same order.  Two
 *                calls on the same input agree bit for bit
 *   x            (B,T,V) emissions, strides sB,sT,sV, E2E_F32 or E2E_F64 (16-bit: up-cast first; E2E_ERR_ARG)
 *   transitions  (V,V) contiguous, x's dtype, or NULL: all zero (a CTC-without-blank model: pass its log-softmax, R = 0)
 *   x_len        (B) int64; x_len[b] outside [1,T] gives n_hyp[b] = 0 and touches nothing else of the utterance
 *   space_id     the space's column among the V - R characters, or negative: none (>= V - R: E2E_ERR_ARG)
 *   lm           NULL or a model of e2e_lm_load_arpa on the current device; order <= 6
 *   nbest        1 <= nbest <= beam_width, else E2E_ERR_ARG
 *   out          (B,nbest,max_out) int64 labels (repeat labels as they are), zero filled behind each sequence; max_out = T
 *                can never be exceeded
 *   out_len      (B,nbest) int64: 0 for slots >= n_hyp[b]; > max_out = truncated, that many ids were needed and the first
 *                max_out were written
 *   n_hyp        (B) int64: min(nbest, members of the final beam)
 *   scores       (B,nbest,3) f64: total, ac, lm_score (0 without a model); slots >= n_hyp[b]: -inf, -inf, 0
 *   counts       (B,nbest,2) int32: num_words, num_oov (0 without a model)
 *   workspace    >= e2e_asg_beam_workspace_bytes(...): 8 V^2 bytes for the transitions as f64, [from][to]; per utterance
 *                20 bytes per (member, label) pair and 8 per node of the pool of beam_width * (T + 1) + 1 (parent, label)
 *                nodes (B=64, T=1000, V=29, beam_width=100: 55 MB).  with_lm does not change it (the LM fields live in LDS)
 * Limits: V <= e2e_asg_max_labels() = 128; beam_width <= e2e_asg_beam_max_width(V) = min(128, 16384 / V), 0 for an
 * unsupported V -- the pair buffers are sized for 16384 pairs, which V <= 128 never exceeds at width 128, so the limit is
 * 128 for every supported V; T <= 2^22.  Beyond them E2E_ERR_UNSUPPORTED (the workspace query returns 0).  Every argument
 * error is found on the host before any launch.  Asynchronous on `stream`, allocates nothing, never synchronises,
 * capturable.  A restriction to the model's vocabulary and label timestamps: e2e_asg_beam_nbest_opt, below the lexicon
 * functions; the same search fed in chunks: e2e_asg_beam_stream, below that.  Not provided: custom transcriptions, a lexicon together with a language model, widths or alphabets
 * above 128.
 */
struct e2e_lm;   /* (e2e_lm_load_arpa, below) */
int e2e_asg_beam_max_width(int V);
size_t e2e_asg_beam_workspace_bytes(int B, int T, int V, int beam_width, int with_lm);

int e2e_asg_beam_nbest(const void* x, int dtype, int64_t sB, int64_t sT, int64_t sV, const void* transitions,
                       const int64_t* x_len, int B, int T, int V, int num_replabels, int beam_width, int space_id,
                       const struct e2e_lm* lm, double lmwt, double wip, double oov_penalty,
                       int nbest, int64_t* out, int64_t max_out, int64_t* out_len, int64_t* n_hyp, double* scores,
                       int32_t* counts, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Greedy decode.  Replaces cpp_ctc_decoder.CTCDecoder.decode_greedy
 *   src/decoders/ctc_decoder.cpp:443-490 (argmax + blank/repeat collapse).
 *   x        (B,T,V) logits or log-probs, strides sB,sT,sV, f32/f64
 *   x_len    (B) int64
 *   out      (B,T) int64, written zero-padded on the right (quirk Q5)
 *   out_len  (B) int64
 */
int e2e_ctc_greedy(const void* x, int dtype, int64_t sB, int64_t sT, int64_t sV,
                   const int64_t* x_len, int B, int T, int V, int blank,
                   int64_t* out, int64_t* out_len, void* stream);

/* ------------------------------------------------------------------------
 * n-gram language model (stands where KenLM's ProbingModel stands in the
 * reference: src/decoders/ctc_decoder.cpp:60-71 load, :77-88 get_idx,
 * :275-278,:291-294 BaseScore).  Host-side ARPA reader (plain or .gz) that
 * builds a device-resident hash table.  `labels` are the decoder's V label
 * strings (UTF-8): words are spelled with them.
 *
 * Hashed matching: on the device a word is found by the 64-bit FNV hash of its
 * spelling and an n-gram by a 64-bit signature of its word ids; the entries keep
 * the hash, not the spelling / ids.  What the model lists is always found.  A
 * query the model does NOT list -- an out-of-vocabulary spelling, an unseen
 * n-gram -- is taken for a listed one if the two hashes collide: about 2^-64
 * per probe, i.e. correct with overwhelming probability, not by construction
 * (KenLM's probing model matches on 64-bit hashes in the same way).  The host
 * scorer below (e2e_lm_score) compares ids and is exact.  A model that lists an
 * n-gram without its context (SRILM-pruned ARPA files) is served from id-keyed
 * tables, which are slower.
 */
typedef struct e2e_lm e2e_lm;
/* Reads the model and uploads its tables to the CURRENT HIP device (this call allocates and synchronises; it is
 * the one entry point that does).  A model serves calls on that device only: load it once per device. */
int e2e_lm_load_arpa(const char* path /* host */, const char* const* labels /* host */, int V,
                     int case_sensitive, e2e_lm** out);
void e2e_lm_free(e2e_lm* lm);
int e2e_lm_order(const e2e_lm* lm);
int e2e_lm_device(const e2e_lm* lm);   /* HIP device index of the tables; -1 = host tables only (no GPU at load) */
/* host-side scoring helpers (testing / print_scores_for_sentence,
 * src/decoders/ctc_decoder.cpp:141-151): word index (0 = <unk>) and
 * log10 p(word | most-recent-first context ids). */
uint32_t e2e_lm_word_index(const e2e_lm* lm, const char* word /* host */);
double e2e_lm_score(const e2e_lm* lm, const uint32_t* ctx /* host */, int ctx_len, uint32_t word);

/* ------------------------------------------------------------------------
 * Prefix beam search.  Replaces cpp_ctc_decoder.CTCDecoder.decode
 *   src/decoders/ctc_decoder.cpp:153-201 (driver), :353-441 (decode_sentence),
 *   :247-312 (get_next_prefix), :314-318 (score).
 *   lp        (B,T,V) LOG-PROBABILITIES, strides sB,sT,sV, f32 / f64 / f16 / bf16 (16-bit values are read as they are: the
 *             search is the one of their f32 images, bit for bit)
 *   space_id  index of " " among the labels, or -1 (:55-59)
 *   lm        NULL for none (lmwt then counts as 0, :72-74); else a model loaded on the current device
 *             with exactly V labels (E2E_ERR_ARG otherwise)
 *   out       (B,max_out) int64, zero-filled; out_len (B) int64.  When the
 *             empty prefix wins the result is the single id -1 (quirk Q6).
 *             Per-utterance status rides on out_len (no separate call, nothing synchronises):
 *               0 <= out_len[b] <= max_out   the sentence is out[b, :out_len[b]]
 *               out_len[b] > max_out         the sentence has out_len[b] ids, only the first max_out were
 *                                            written (max_out = x_len[b] + 1 can never be exceeded)
 *               out_len[b] == -1             the prefix-tree node pool ran out (cannot happen with a workspace
 *                                            of e2e_ctc_beam_workspace_bytes(); the row must not be used)
 *   workspace >= e2e_ctc_beam_workspace_bytes(...)
 * Limits (E2E_ERR_UNSUPPORTED beyond them; the reference has none): beam_width <= e2e_ctc_beam_max_width() = 512,
 * language models of order <= 6.
 */
size_t e2e_ctc_beam_workspace_bytes(int B, int T, int V, int beam_width);
/* The same for a caller that knows whether the call will carry a language model (with_lm 0 / 1): only what that call needs --
 * without a model the general kernel's rows of LM answers are left out, and nothing of the general kernel's is counted where
 * the one-workgroup kernel takes the call.  e2e_ctc_beam_workspace_bytes() is the larger of the two. */
size_t e2e_ctc_beam_workspace_bytes_lm(int B, int T, int V, int beam_width, int with_lm);
/* The largest beam_width e2e_ctc_beam accepts for an alphabet of V columns, with or without a language model: 512 for
 * any V.  Two kernels stand behind the call: the fast one keeps everything that scales with beam_width * V in one
 * workgroup's LDS (V = 29: widths up to 150, 103 with an LM; V = 80: 81 / 47); beyond that the general kernel keeps the
 * candidate keys and the LM's answers in the workspace (any V, e.g. the reference's default width 100 at V = 8000) --
 * same result, slower per step; beyond ~256 hypotheses it also keeps the beam members' state there.  Host callers check the width at construction instead of failing at the first decode. */
int e2e_ctc_beam_max_width(int V, int with_lm);

int e2e_ctc_beam(const void* lp, int dtype, int64_t sB, int64_t sT, int64_t sV,
                 const int64_t* x_len, int B, int T, int V, int blank,
                 int beam_width, int space_id, const e2e_lm* lm,
                 double lmwt, double wip, double oov_penalty,
                 int64_t* out, int64_t max_out, int64_t* out_len,
                 void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------
 * The same search, read out as an n-best list (additive, ABI 4: nothing above changes meaning).
 * The search ends with up to beam_width ranked hypotheses; e2e_ctc_beam returns the first, this call the first `nbest`,
 * ranked as the search ranks its own candidates: total score descending, ties (and -inf scores) by position in the final
 * beam.  Hypothesis 0 is e2e_ctc_beam's result, bit for bit.  Arguments up to oov_penalty, dtypes, strides, width limits
 * and language-model rules are e2e_ctc_beam's; asynchronous, allocates nothing, capturable.
 *   nbest      1 <= nbest <= beam_width, else E2E_ERR_ARG (as is a beam_width above e2e_ctc_beam_max_width(): every
 *              argument error is found on the host before any launch)
 *   out        (B,nbest,max_out) int64, zero-filled behind each sentence
 *   out_len    (B,nbest) int64: 0 for slots >= n_hyp[b]; > max_out = truncated, that many ids were needed and the first
 *              max_out were written (the in-band status of e2e_ctc_beam, per hypothesis)
 *   n_hyp      (B) int64: min(nbest, members of the final beam); -1 = the node pool ran out (nothing of the utterance may
 *              be used)
 *   scores     (B,nbest,3) f64: total (what the search ranks by), its CTC part log(p_blank + p_non_blank), the
 *              language model's score (0 without a model); total = ctc + lmwt * lm - wip * num_words + oov_penalty *
 *              num_oov.  Slots >= n_hyp[b]: -inf, -inf, 0.
 *   counts     (B,nbest,2) int32: num_words, num_oov (0 without a model)
 *   timesteps  NULL, or (B,nbest,max_out) int64: for every id written to `out` the frame at which the prefix ending in
 *              that label was created, i.e. entered the beam on this path (a prefix is created once and never re-created);
 *              strictly increasing along a sentence; -1 behind the sentence and for the -1 id of an empty winner.
 *              Only a call with timesteps records the frames: one int32 per prefix-tree node more workspace.
 *   workspace >= e2e_ctc_beam_nbest_workspace_bytes(...); with_timesteps = 0: exactly e2e_ctc_beam_workspace_bytes_lm().
 */
size_t e2e_ctc_beam_nbest_workspace_bytes(int B, int T, int V, int beam_width, int with_lm, int with_timesteps);

int e2e_ctc_beam_nbest(const void* lp, int dtype, int64_t sB, int64_t sT, int64_t sV,
                       const int64_t* x_len, int B, int T, int V, int blank,
                       int beam_width, int space_id, const e2e_lm* lm,
                       double lmwt, double wip, double oov_penalty,
                       int nbest, int64_t* out, int64_t max_out, int64_t* out_len, int64_t* n_hyp,
                       double* scores, int32_t* counts, int64_t* timesteps,
                       void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Beam search restricted to a vocabulary (additive, ABI 4: nothing above changes meaning).
 *
 * The lexicon L of a model is the set of its words -- the unigrams but <unk>, <s> and </s> -- spelled as the lookup of a
 * beam's words spells them: the labels' UTF-8 bytes, A-Z folded unless the model is case sensitive.  Pref(L) is every
 * non-empty byte prefix of a word of L, the words included.  A restricted search creates a prefix's child only if
 *   - the character is no space and the child's last word is spelled in Pref(L), or
 *   - the character is the space and the prefix is the root, ends in a space, or ends in a word of L.
 * A child that is alive already is found as ever (quirk Q7 included); a pair without a child gives the child nothing and
 * creates no candidate, while the prefix's own repeated-character share is taken as ever.  Scores, selection and tie order
 * are the unrestricted search's.  The last word of a hypothesis may be a prefix that is no word: it counts as out of
 * vocabulary, as it always did.
 *
 * e2e_lm_load_words      a model that scores nothing, from a word list (host strings without white space): order 1, every
 *                        word and <unk> at log10 p = 0, <unk> = id 0, <s> and </s> present.  Unrestricted, with
 *                        oov_penalty = 0, its search is the search without a model, bit for bit.  Uploads like
 *                        e2e_lm_load_arpa.
 * e2e_lm_enable_lexicon  builds the lexicon of a model and uploads it: the prefixes that are no words enter the vocabulary
 *                        tables with id 0, so the probe that finds a word's id also answers "may this spelling go on?".
 *                        Allocates and synchronises like the loader (no call may be in flight on the model); idempotent.
 *                        Unrestricted calls compute what they computed before.  A model whose lexicon was never asked for
 *                        keeps the tables it always had.  E2E_ERR_UNSUPPORTED if the labels can spell <unk>, <s> or </s>
 *                        inside the lexicon (the tables hold those three, and could not tell them from words).
 * e2e_lm_has_lexicon     1 once e2e_lm_enable_lexicon has succeeded.
 * e2e_lm_spelling_class  host helper: bit 0 = the spelling is a word of L, bit 1 = it is a proper prefix of a longer word;
 *                        0 for a model without a lexicon.
 * e2e_ctc_beam_nbest_opt e2e_ctc_beam_nbest with options.  opts == NULL or restrict_to_lexicon == 0 is e2e_ctc_beam_nbest
 *                        exactly.  restrict_to_lexicon != 0 with lm == NULL or a model without a lexicon is E2E_ERR_ARG, found
 *                        before any launch.  Workspace, width limits and outputs are e2e_ctc_beam_nbest's.
 */
int e2e_lm_load_words(const char* const* words /* host */, int n_words, const char* const* labels /* host */, int V,
                      int case_sensitive, e2e_lm** out);
int e2e_lm_enable_lexicon(e2e_lm* lm);
int e2e_lm_has_lexicon(const e2e_lm* lm);
int e2e_lm_spelling_class(const e2e_lm* lm, const char* spelling /* host */);

typedef struct e2e_ctc_beam_opts {
  int restrict_to_lexicon;   /* 0: the plain search */
} e2e_ctc_beam_opts;

int e2e_ctc_beam_nbest_opt(const void* lp, int dtype, int64_t sB, int64_t sT, int64_t sV,
                           const int64_t* x_len, int B, int T, int V, int blank,
                           int beam_width, int space_id, const e2e_lm* lm,
                           double lmwt, double wip, double oov_penalty,
                           int nbest, int64_t* out, int64_t max_out, int64_t* out_len, int64_t* n_hyp,
                           double* scores, int32_t* counts, int64_t* timesteps,
                           void* workspace, size_t workspace_bytes, void* stream, const e2e_ctc_beam_opts* opts);

/* ------------------------------------------------------------------------
 * ASG beam search restricted to a vocabulary, and label timestamps (additive, ABI 4: nothing above changes meaning).
 *
 * e2e_asg_beam_nbest_opt is e2e_asg_beam_nbest with options; opts == NULL, or both fields zero, is e2e_asg_beam_nbest bit
 * for bit.  Workspace (e2e_asg_beam_workspace_bytes), width and alphabet limits, outputs, ranking and tie order do not change.
 *
 * restrict_to_lexicon   L and Pref(L) are those of e2e_ctc_beam_nbest_opt: the model's words, folded as the lookup folds them,
 *                       and every non-empty byte prefix of a word.  The LAST WORD of a sequence is the run of labels after its
 *                       last space, spelled with repeat labels expanded, exactly as the LM lookup of e2e_asg_beam_nbest spells
 *                       it.  A sequence is ADMISSIBLE if it is spellable and every one of its prefixes y + (c) obeys:
 *                         - c is not the space: the last word of y + (c) is spelled in Pref(L);
 *                         - c is the space: y is empty, or the last word of y is a word of L.
 *                       A restricted search forms only admissible sequences: an inadmissible y + (c) is no candidate at frame 0
 *                       and no extension later, like an unspellable one.  Admissibility is a function of the sequence alone, so
 *                       the cut and the re-formation rule are untouched; masses, LM fields, totals, cut and ranking are the
 *                       unrestricted search's.  The last word of a hypothesis may be a proper prefix that is no word: it counts
 *                       as out of vocabulary, as it always did.  Spellings are not canonicalised: a <2> and a <1> a remain two
 *                       sequences.  With num_replabels = 0 a word with a doubled letter cannot be spelled (equal neighbours
 *                       merge), so a restricted search never produces it.
 *                       != 0 with lm == NULL or a model without a lexicon (e2e_lm_enable_lexicon): E2E_ERR_ARG, before any
 *                       launch.  A transcription model stays refused (E2E_ERR_UNSUPPORTED).
 * timesteps             NULL, or (B,nbest,max_out) int64: for every id written to `out`, the frame at which the pool node that
 *                       carries it was created -- the frame at which the sequence ending in that label last entered the beam on
 *                       this path, (node - 1) / beam_width, read during the read-out's backward walk: no workspace, no per-frame
 *                       work.  Along a sequence the values increase strictly; the first is 0 (a one-label sequence is only
 *                       formed at frame 0); entry k is >= k and < x_len[b]; behind the sequence and in slots >= n_hyp[b]: -1.
 *                       x_len[b] outside [1,T] leaves the utterance's timesteps untouched, like everything else of it.
 *                       The caveat of e2e_ctc_beam_nbest's timesteps holds here too: in a wide beam a sequence can enter the
 *                       beam before its last label becomes likely, so a value can precede the frame where the label is heard.
 */
typedef struct e2e_asg_beam_opts {
  int restrict_to_lexicon;   /* 0: the plain search */
  int64_t* timesteps;        /* NULL, or (B,nbest,max_out) int64 */
} e2e_asg_beam_opts;

int e2e_asg_beam_nbest_opt(const void* x, int dtype, int64_t sB, int64_t sT, int64_t sV, const void* transitions,
                           const int64_t* x_len, int B, int T, int V, int num_replabels, int beam_width, int space_id,
                           const e2e_lm* lm, double lmwt, double wip, double oov_penalty,
                           int nbest, int64_t* out, int64_t max_out, int64_t* out_len, int64_t* n_hyp, double* scores,
                           int32_t* counts, void* workspace, size_t workspace_bytes, void* stream,
                           const e2e_asg_beam_opts* opts);

/* ------------------------------------------------------------------------
 * Streaming ASG beam search: e2e_asg_beam_nbest_opt fed in chunks, the beam kept on the device between the calls (additive,
 * ABI 4: nothing above changes meaning).  The conventions are e2e_ctc_beam_stream's.
 *
 * An utterance's search lives in one STATE ROW of device memory that the caller owns.  Its parts, each rounded up to 256
 * bytes: a 256-byte header (a magic value; the configuration V, num_replabels, beam_width, model or not, max_frames; the
 * member count, the frames consumed, whether the beam is dead), the beam's current members (log mass, key, last label, node,
 * length, word count: 4096 bytes), with a model their language-model fields (10240 bytes), and the pool of
 * beam_width * (max_frames + 1) + 1 (parent, label) nodes of 8 bytes.  A call resumes every utterance from its row, runs
 * chunk_len[b] further frames, stores the row and reads the current beam out.  What a frame rebuilds anyway is not stored:
 * the members' key table is refilled from their keys at resume, the pair buffers are a frame's scratch.  A node's index,
 * 1 + frame * beam_width + rank, counts the frames of the STREAM, so the timesteps need no storage.  The transitions are not
 * part of the row: the caller passes them with every chunk.
 *   - A row whose first 256 bytes are zero is a fresh utterance: hipMemsetAsync (or zeroing the header) opens or resets a
 *     stream, no other call is needed.  The rest of a fresh row may hold anything.
 *   - Rows are self-contained: indices, no addresses.  They may be moved, permuted, gathered or reordered between calls,
 *     and a batch may mix fresh rows with rows of any age.
 *   - The call is asynchronous on `stream`, allocates nothing, does not synchronise and is capturable.
 *   - Every argument error the host can see is found before any launch, with e2e_asg_beam_nbest_opt's codes: the dtype,
 *     sizes, the alphabet and width limits (E2E_ERR_UNSUPPORTED), num_replabels, space_id, nbest outside [0, beam_width],
 *     max_frames outside [1, 2^22], row_bytes below the query or no multiple of 8, the language model's alphabet, order
 *     and device (a model with transcriptions stays refused, E2E_ERR_UNSUPPORTED), restrict_to_lexicon without a lexicon,
 *     null pointers, the workspace's size (E2E_ERR_WORKSPACE).
 * CONTRACT.  After chunks whose lengths for utterance b sum to f_b >= 1 -- fed with the same transitions, beam_width, model,
 * lmwt / wip / oov_penalty and options throughout -- every output of the read-out (out, out_len, n_hyp, scores, counts,
 * opts->timesteps) equals, bit for bit, what e2e_asg_beam_nbest_opt writes for the concatenated frames with x_len[b] = f_b
 * and the same nbest, max_out and options.  Timesteps are frames of the stream, not of the chunk.  A beam that died (no
 * candidate with a number for a total: n_hyp = 0, lengths 0, totals -inf) stays dead over later chunks and reads out as the
 * whole call does.  f_b = 0 (a fresh row fed no frames): n_hyp[b] = 0, frames_done[b] = 0 and nothing else of the
 * utterance is written, as the whole call leaves an utterance alone whose length is outside [1,T].
 *   x            (B,T,V) emissions of this chunk, strides sB,sT,sV, E2E_F32 or E2E_F64 (chunks may differ in dtype; the
 *                transitions have the chunk's)
 *   transitions  (V,V) contiguous, x's dtype, or NULL: all zero; the same values with every chunk
 *   chunk_len    (B) int64, device: frames of this chunk per utterance, clamped to 0..T.  0 runs no frame and stores
 *                nothing: the read-out repeats the utterance's last result
 *   state        (B,row_bytes) device, 8-byte aligned; row_bytes >= e2e_asg_beam_stream_row_bytes(...), a multiple of 8
 *   max_frames   the longest stream a row can hold, 1 .. 2^22; part of the row's configuration, checked at resume
 *   nbest        0: feed only, no read-out: the outputs up to counts (and opts->timesteps) may be NULL and are not touched;
 *                else 1 .. beam_width as in e2e_asg_beam_nbest
 *   frames_done  (B) int64, device.  What only the device knows is reported here per utterance, and mirrored in n_hyp[b]
 *                when nbest > 0:
 *                  >= 0  frames consumed so far
 *                  -2    this chunk would pass max_frames
 *                  -3    the row was not written under this configuration
 *                Both statuses are found before anything of the row is touched: they leave the whole row byte for byte and
 *                write none of the utterance's other outputs, and the other utterances advance.  There is no -1: the pool
 *                is sized exactly.
 *   workspace    >= e2e_asg_beam_stream_workspace_bytes(...): 8 V^2 bytes for the transitions as f64, [from][to], and per
 *                utterance 20 bytes per (member, label) pair.  It does not depend on the frames: the node pool is the row's
 *   opts         NULL or e2e_asg_beam_opts as in e2e_asg_beam_nbest_opt; restrict_to_lexicon the same for every chunk,
 *                timesteps NULL or (B,nbest,max_out) per call
 * Row size: 256 + 4096 + (10240 with_lm) + 8 * (beam_width * (max_frames + 1) + 1) rounded up to 256; 0 for a width,
 * alphabet or max_frames that is not supported.  beam_width 100, max_frames 30 000: 24 005 376 bytes (24 015 616 with a
 * model) per utterance, whatever the alphabet: 24 MB, the node pool being all but 4 KB (14 KB) of it.
 */
size_t e2e_asg_beam_stream_row_bytes(int max_frames, int V, int beam_width, int with_lm);
size_t e2e_asg_beam_stream_workspace_bytes(int B, int V, int beam_width, int with_lm);

int e2e_asg_beam_stream(const void* x, int dtype, int64_t sB, int64_t sT, int64_t sV, const void* transitions,
                        const int64_t* chunk_len, int B, int T, int V, int num_replabels, int beam_width, int space_id,
                        const e2e_lm* lm, double lmwt, double wip, double oov_penalty,
                        void* state, size_t row_bytes, int max_frames,
                        int nbest, int64_t* out, int64_t max_out, int64_t* out_len, int64_t* n_hyp, double* scores,
                        int32_t* counts, int64_t* frames_done,
                        void* workspace, size_t workspace_bytes, void* stream, const e2e_asg_beam_opts* opts);

/* ------------------------------------------------------------------------
 * ASG beam search with per-frame label pruning (cutoff_top_n; flashlight's beam_size_token) -- additive, ABI 4: nothing
 * above changes meaning.  e2e_asg_beam_nbest_cut is e2e_asg_beam_nbest_opt, e2e_asg_beam_stream_cut is e2e_asg_beam_stream,
 * each with one more argument.
 *
 * DEFINITION.  For a frame's row x[t, 0..V) as the search reads it (f32 / f64) and cutoff_top_n >= 1:
 *   1. order the labels by x descending, ties by label id ascending; NaN counts as -inf, -0 and +0 are one number;
 *   2. K = min(cutoff_top_n, V); the frame's kept set is the first K of that order, written in ascending id.
 * There is no always-kept label -- ASG has no blank -- so a frame keeps exactly K labels.  There is no cutoff_prob: ASG
 * emissions are scores, not log-probabilities, and sum exp(x) means nothing for them (nor is a softmax of them defined here).
 * In the search a label outside the frame's kept set does nothing in that frame:
 *   - it is no candidate at frame 0;
 *   - it gives no extension share, from any member;
 *   - a member whose last label is not kept gets no stay share: it survives the frame only as a parent.
 * Everything else is e2e_asg_beam_nbest_opt's: spellability and the restriction rule, the two-term symmetric log-sum,
 * identity by key and ranking by key, the LM fields, the node numbering 1 + t * beam_width + rank and with it the timesteps,
 * and the "no hypothesis left" end (n_hyp = 0, a stream's header dead) -- which pruning makes likelier: with K = 1 a frame
 * whose one kept label no member can stay on or take ends the search.
 * CONSEQUENCE.  A pruned call equals, bit for bit in every output (ids, lengths, n_hyp, scores, counts, timesteps,
 * frames_done), the unpruned call on emissions whose non-kept columns are replaced by -inf: an extension or stay share of a
 * -inf emission is -inf, the symmetric log-sum of -inf and v is v, and a -inf total is no candidate.
 * cutoff_top_n >= V is no pruning: the *_cut entries then are the unpruned entries -- the same kernel, the same workspace.
 *
 *   limits     V <= e2e_asg_max_labels(), beam_width <= e2e_asg_beam_max_width(V): the unpruned ones
 *   workspace  >= e2e_asg_beam_cut_workspace_bytes(...) (a stream: e2e_asg_beam_cut_stream_workspace_bytes, T the chunk's):
 *              the frames' lists, (B,T,K) and (B,T) int32; 8 V^2 bytes for the transitions as f64; per utterance the pair
 *              buffers of e2e_asg_beam_nbest with K in V's place; for a whole call the node pool.  A query returns 0 where
 *              the call would be refused, and the unpruned query's value for cutoff_top_n >= V
 *   a stream   cutoff_top_n is the same for every chunk (the caller's contract, as for opts); the selection runs on each
 *              chunk; the state row and its header are e2e_asg_beam_stream_row_bytes', unchanged; after any chunking the
 *              read-out equals the whole pruned call, bit for bit
 * Argument errors are found on the host before any launch: cutoff_top_n < 1 is E2E_ERR_ARG, a workspace that is too small
 * E2E_ERR_WORKSPACE, everything else as for the unpruned entries.  The selection, the transposition and the search run on
 * `stream` in one call: asynchronous, allocates nothing, never synchronises, capturable.
 */
size_t e2e_asg_beam_cut_workspace_bytes(int B, int T, int V, int beam_width, int with_lm, int cutoff_top_n);
size_t e2e_asg_beam_cut_stream_workspace_bytes(int B, int T, int V, int beam_width, int with_lm, int cutoff_top_n);

int e2e_asg_beam_nbest_cut(const void* x, int dtype, int64_t sB, int64_t sT, int64_t sV, const void* transitions,
                           const int64_t* x_len, int B, int T, int V, int num_replabels, int beam_width, int space_id,
                           const e2e_lm* lm, double lmwt, double wip, double oov_penalty,
                           int nbest, int64_t* out, int64_t max_out, int64_t* out_len, int64_t* n_hyp, double* scores,
                           int32_t* counts, void* workspace, size_t workspace_bytes, void* stream,
                           const e2e_asg_beam_opts* opts, int cutoff_top_n);

int e2e_asg_beam_stream_cut(const void* x, int dtype, int64_t sB, int64_t sT, int64_t sV, const void* transitions,
                            const int64_t* chunk_len, int B, int T, int V, int num_replabels, int beam_width, int space_id,
                            const e2e_lm* lm, double lmwt, double wip, double oov_penalty,
                            void* state, size_t row_bytes, int max_frames,
                            int nbest, int64_t* out, int64_t max_out, int64_t* out_len, int64_t* n_hyp, double* scores,
                            int32_t* counts, int64_t* frames_done,
                            void* workspace, size_t workspace_bytes, void* stream, const e2e_asg_beam_opts* opts,
                            int cutoff_top_n);

/* ------------------------------------------------------------------------
 * Custom transcriptions: a pronunciation lexicon, homophones included (additive, ABI 4: nothing above changes meaning).
 *
 * A transcription lexicon is a list of entries (word, t_1 .. t_k), k >= 1, every t_i a label of the decoder that is neither
 * the blank nor the space.  A word may have several entries (variants); a transcription may belong to several words
 * (homophones).  A model loaded with one finds a prefix's last word by its sequence of label IDS between two spaces, not by
 * the labels' strings: with labels A, AH, HK, K the transcriptions "A HK" and "AH K" are different keys.  Everything else
 * of the search -- e2e_ctc_beam, _nbest, _nbest_opt, _stream -- is what it was.
 *   - Wd(s) is the set of the model's words with transcription s, in the order of their first entry.  The word of a child
 *     whose last word is transcribed s is the w in Wd(s) with the greatest log10 p(w | the LM state before the word), the f32
 *     value the search's own LM walk computes; exact ties go to the earliest of Wd(s).  Its LM score, LM state and
 *     out-of-vocabulary count are that word's.  The choice is made again at every label, from the state before the word.
 *   - A transcription that is no key, or only a proper prefix of one, is <unk> (id 0, out of vocabulary).
 *   - Restricted to the lexicon (e2e_lm_enable_lexicon, restrict_to_lexicon): L is the set of kept transcriptions, Pref(L)
 *     their non-empty prefixes on label boundaries; the rule above holds on these.
 * Limits: a transcription has at most 255 labels; at most 16 words share one (E2E_ERR_UNSUPPORTED beyond either); the word
 * boundary is the label " "; at most 65535 labels; LM order <= 6.  <unk>, <s> and </s> have no transcription (E2E_ERR_ARG as an entry's word).
 * e2e_asg_beam refuses such a model (E2E_ERR_UNSUPPORTED).
 *
 * e2e_lm_load_transcriptions     path: an ARPA file (as e2e_lm_load_arpa), or NULL for the model that scores nothing over the
 *                                entries' words (as e2e_lm_load_words: homophones always tie, the first listed wins).
 *                                entry_words[i] is entry i's word; its label ids are entry_label_ids[entry_off[i] ..
 *                                entry_off[i+1]) (all host).  Words are matched to the model's as e2e_lm_word_index matches
 *                                them (lower-cased on both sides unless case_sensitive).  With an ARPA file an entry whose
 *                                word the model does not list is dropped.  E2E_ERR_ARG, naming the entry, for an empty
 *                                lexicon, an entry without labels, an id outside [0, V) or the space as a token.  (The blank
 *                                is not known here: the caller keeps it out of the entries.)  Uploads like e2e_lm_load_arpa
 *                                and also works with no GPU (e2e_lm_device == -1).
 * e2e_lm_is_transcribed          1 for a model of e2e_lm_load_transcriptions.  On such a model e2e_lm_word_index still takes a
 *                                word's string; e2e_lm_spelling_class, which takes a spelling, answers 0.
 * e2e_lm_transcriptions_dropped  the number of entries dropped at load.
 * e2e_lm_transcribe              host helper: the words of a label sequence as the search reads them.  ids (host, n of them) is
 *                                split at space_id, empty pieces skipped; every piece is looked up and a homophone set is
 *                                resolved in the running context with the host scorer, starting behind <s>.  Writes at most
 *                                max_words word ids (0 = <unk>: no key) and the number of pieces to *n_words.  Works on every
 *                                model: one without transcriptions spells the pieces from the labels' strings.
 * e2e_lm_word_string             the word of an id as the model lists it (owned by the model), NULL for an id it has not.
 */
int e2e_lm_load_transcriptions(const char* path /* host or NULL */, const char* const* entry_words /* host */,
                               const int32_t* entry_label_ids /* host */, const int32_t* entry_off /* host, n_entries + 1 */,
                               int n_entries, const char* const* labels /* host */, int V, int case_sensitive, e2e_lm** out);
int e2e_lm_is_transcribed(const e2e_lm* lm);
int e2e_lm_transcriptions_dropped(const e2e_lm* lm);
int e2e_lm_transcribe(const e2e_lm* lm, const int64_t* ids /* host */, int64_t n, int space_id,
                      uint32_t* word_ids_out /* host */, int max_words, int* n_words /* host */);
const char* e2e_lm_word_string(const e2e_lm* lm, uint32_t id);

/* ------------------------------------------------------------------------
 * Streaming beam search: the same search fed in chunks, the beam kept on the device between the calls (additive, ABI 4:
 * nothing above changes meaning).
 *
 * An utterance's search lives in one STATE ROW of device memory that the caller owns: a 256-byte header, the beam's members
 * (probabilities, prefix, guard, language-model state), the prefix-tree node pool of max_frames frames and, with_timesteps,
 * one int32 per node.  A call resumes every utterance from its row, consumes chunk_len[b] further frames, stores the row
 * and reads the current beam out.  What a step rebuilds anyway is not stored: the node -> position map, the child tables
 * (from the members' guards) and the language model's answers (asked again at resume: they are a function of a member's
 * state, and the row stays independent of the alphabet).
 *   - A row whose first 256 bytes are zero is a fresh utterance: hipMemsetAsync (or zeroing the header) opens or resets a
 *     stream, no other call is needed.  The rest of a fresh row may hold anything.
 *   - Rows are self-contained: indices, no addresses.  They may be moved, gathered or reordered between calls, and a batch
 *     may mix fresh rows with rows of any age.
 *   - The call is asynchronous on `stream`, allocates nothing, does not synchronise and is capturable.
 *   - Every argument error the host can see is E2E_ERR_ARG before any launch: sizes, null pointers, row_bytes below the
 *     query, nbest outside [0, beam_width], the width limit, the language model's device / alphabet, restrict_to_lexicon
 *     without a lexicon, timesteps != NULL with with_timesteps == 0.
 * CONTRACT.  After chunks whose lengths for utterance b sum to f_b, every output of the read-out -- out, out_len, n_hyp,
 * scores, counts, timesteps -- equals, bit for bit, what e2e_ctc_beam_nbest_opt writes for the concatenated frames with
 * x_len[b] = f_b and the same nbest, max_out and options.  Timestamps are frames of the whole stream, not of the chunk.
 *   lp           (B,T,V) log-probabilities of this chunk, strides sB,sT,sV, any of the four dtypes (chunks may differ)
 *   chunk_len    (B) int64, device: frames of this chunk per utterance, clamped to 0..T.  0 runs no step and stores
 *                nothing: the read-out repeats the utterance's last result (a fresh row: the root's)
 *   state        (B,row_bytes) device, 8-byte aligned; row_bytes >= e2e_ctc_beam_stream_row_bytes(...), a multiple of 8
 *   max_frames   the longest stream a row can hold; V, beam_width, lm or not, max_frames and with_timesteps are the row's
 *                configuration and are checked against the header at resume
 *   nbest        0: feed only, no read-out, the outputs up to timesteps may be NULL and are not touched; else as in
 *                e2e_ctc_beam_nbest (1 gives e2e_ctc_beam's result as hypothesis 0)
 *   max_out      as in e2e_ctc_beam_nbest; f_b + 1 can never be exceeded
 *   frames_done  (B) int64, device.  What only the device knows is reported here per utterance, and mirrored in n_hyp[b]
 *                when nbest > 0:
 *                  >= 0  frames consumed so far
 *                  -1    the node pool ran out (cannot happen within max_frames)
 *                  -2    this chunk would pass max_frames
 *                  -3    the row was not written under this configuration
 *                A status < 0 leaves the row's header and members as they were (-2 and -3: the whole row, byte for byte;
 *                the utterance's other outputs are then not written), and the other utterances advance.
 *   workspace    >= e2e_ctc_beam_stream_workspace_bytes(...): the general kernel's scratch only (0, and NULL allowed,
 *                where the one-workgroup kernel takes the width; the choice does not depend on the frames)
 *   opts         NULL, or e2e_ctc_beam_opts as in e2e_ctc_beam_nbest_opt; the same for every chunk of a stream
 * Row size: 256 + 176 * beam_width + (beam_width * (max_frames + 3) + 8) * (8, or 12 with_timesteps), each part rounded up
 * to 256: beam_width 100, max_frames 30 000: 24 MB (36 MB) per utterance, whatever the alphabet.
 */
size_t e2e_ctc_beam_stream_row_bytes(int max_frames, int V, int beam_width, int with_lm, int with_timesteps);
size_t e2e_ctc_beam_stream_workspace_bytes(int B, int V, int beam_width, int with_lm);

int e2e_ctc_beam_stream(const void* lp, int dtype, int64_t sB, int64_t sT, int64_t sV,
                        const int64_t* chunk_len, int B, int T, int V, int blank,
                        int beam_width, int space_id, const e2e_lm* lm,
                        double lmwt, double wip, double oov_penalty,
                        void* state, size_t row_bytes, int max_frames, int with_timesteps,
                        int nbest, int64_t* out, int64_t max_out, int64_t* out_len, int64_t* n_hyp,
                        double* scores, int32_t* counts, int64_t* timesteps, int64_t* frames_done,
                        void* workspace, size_t workspace_bytes, void* stream, const e2e_ctc_beam_opts* opts);

/* ------------------------------------------------------------------------
 * Per-frame label pruning (cutoff_top_n, cutoff_prob) -- an extension (no counterpart upstream; the knobs of parlance
 * ctcdecode, PaddlePaddle DeepSpeech, pyctcdecode, flashlight).  Additive, ABI 4.
 *
 * DEFINITION.  For a frame's row lp[0..V), taken as the numbers the search reads (16-bit inputs as their f32 images), and
 * cutoff_top_n >= 1, 0 < cutoff_prob <= 1:
 *   1. order the labels by lp descending, ties by label id ascending; NaN counts as -inf;
 *   2. K = min(cutoff_top_n, V); take the first K of that order;
 *   3. if cutoff_prob < 1: with P_j the f64 sum of exp(lp) over the first j, keep the first k, the smallest j with
 *      P_j >= cutoff_prob, or all K if there is none.  cutoff_prob == 1 skips this step exactly: no sum is compared with 1;
 *   4. the blank is always kept: if it is not among the k it is added and uses none of the K places, so a frame keeps
 *      between 1 and k + 1 labels;
 *   5. the kept set is written in ascending label id, the order in which the search expands it.
 * In the search a label outside the frame's set does nothing in that frame: it creates no child, gives no share to a living
 * child and no repeated-label share to the member itself.  Everything else is e2e_ctc_beam_nbest_opt's.
 * cutoff_top_n >= V together with cutoff_prob == 1 is no pruning: the *_cut calls are then the unpruned calls.
 * (P_j is summed by a scan of fixed shape, not one label after the other: a frame whose P_j comes within a few ulp of
 * cutoff_prob may keep one label more or fewer than a sequential sum would; a call repeats bit for bit.)
 *
 * e2e_ctc_label_cut: the selection alone, one kernel over the B*T frames.
 *   lp, dtype, sB, sT, sV, x_len, B, T, V, blank   as e2e_ctc_beam (E2E_F32 / F64 / F16 / BF16, any strides)
 *   ids        (B,T,K+1) int32: a frame's kept labels ascending, -1 behind them
 *   n          (B,T) int32: how many; 0 for t >= x_len[b] (the frame's ids are then not written)
 *   workspace  >= e2e_ctc_label_cut_workspace_bytes(...) (the selection works in LDS: a token block, not read)
 * Limits: min(cutoff_top_n, V) <= e2e_ctc_label_cut_max() = 1024, E2E_ERR_UNSUPPORTED beyond; any V.  Argument errors
 * (sizes, null pointers, cutoff_top_n < 1, cutoff_prob outside (0, 1], blank outside [0, V)) are E2E_ERR_ARG before any
 * launch.  Asynchronous on `stream`, allocates nothing, capturable.
 *
 * e2e_ctc_beam_nbest_cut / e2e_ctc_beam_stream_cut: e2e_ctc_beam_nbest_opt / e2e_ctc_beam_stream with the two knobs; the
 * selection and the search run on `stream` in one call.  A pruned call always takes the general kernel (beam_width <=
 * e2e_ctc_beam_cut_max_width(V, with_lm)); nothing of a frame's work scales with V, and the workspace
 * (e2e_ctc_beam_cut_workspace_bytes; a stream: e2e_ctc_beam_cut_stream_workspace_bytes, T the chunk's) holds the frames'
 * lists and beam_width * (K + 2) candidate keys per utterance instead of beam_width * (V + 1) keys and the LM's answer rows.
 * A stream: the knobs are the same for every chunk (the caller's contract, as for opts), the selection runs on each chunk,
 * the state row is e2e_ctc_beam_stream_row_bytes' unchanged, and the CONTRACT above holds: after any chunking the read-out
 * equals the whole pruned call, bit for bit.
 */
int e2e_ctc_label_cut_max(void);
size_t e2e_ctc_label_cut_workspace_bytes(int B, int T, int V, int cutoff_top_n);
int e2e_ctc_label_cut(const void* lp, int dtype, int64_t sB, int64_t sT, int64_t sV, const int64_t* x_len,
                      int B, int T, int V, int blank, int cutoff_top_n, double cutoff_prob,
                      int32_t* ids, int32_t* n, void* workspace, size_t workspace_bytes, void* stream);

int e2e_ctc_beam_cut_max_width(int V, int with_lm);
size_t e2e_ctc_beam_cut_workspace_bytes(int B, int T, int V, int beam_width, int with_lm, int with_timesteps, int cutoff_top_n);
size_t e2e_ctc_beam_cut_stream_workspace_bytes(int B, int T, int V, int beam_width, int with_lm, int cutoff_top_n);

int e2e_ctc_beam_nbest_cut(const void* lp, int dtype, int64_t sB, int64_t sT, int64_t sV,
                           const int64_t* x_len, int B, int T, int V, int blank,
                           int beam_width, int space_id, const e2e_lm* lm,
                           double lmwt, double wip, double oov_penalty,
                           int nbest, int64_t* out, int64_t max_out, int64_t* out_len, int64_t* n_hyp,
                           double* scores, int32_t* counts, int64_t* timesteps,
                           void* workspace, size_t workspace_bytes, void* stream, const e2e_ctc_beam_opts* opts,
                           int cutoff_top_n, double cutoff_prob);

int e2e_ctc_beam_stream_cut(const void* lp, int dtype, int64_t sB, int64_t sT, int64_t sV,
                            const int64_t* chunk_len, int B, int T, int V, int blank,
                            int beam_width, int space_id, const e2e_lm* lm,
                            double lmwt, double wip, double oov_penalty,
                            void* state, size_t row_bytes, int max_frames, int with_timesteps,
                            int nbest, int64_t* out, int64_t max_out, int64_t* out_len, int64_t* n_hyp,
                            double* scores, int32_t* counts, int64_t* timesteps, int64_t* frames_done,
                            void* workspace, size_t workspace_bytes, void* stream, const e2e_ctc_beam_opts* opts,
                            int cutoff_top_n, double cutoff_prob);

/* ------------------------------------------------------------------------
 * Viterbi forced alignment on the same lattice (max-plus instead of sum).
 * Replaces pytorch_end2end/utils/alignment.py:50-106 (_get_alignment_ctc_1d), :10-47
 * (_get_alignment_asg_1d, is_ctc = 0: no blanks) and the batch driver :109-138
 * (get_alignment_3d), which run as numba-jitted Python on the host upstream.
 *   lp        (B,T,V) LOG-PROBABILITIES, strides sB,sT,sV, f32 / f64 / f16 / bf16 (alpha is f64 either way, as upstream)
 *   targets   (B,*) int64, first t_len[b] entries used; x_len, t_len (B) int64
 *   blank     the blank id (upstream hard-codes 0, :57); ignored when is_ctc = 0
 *   out       (B,T) int64: out[b, t] = the label (or blank) frame t is aligned to for t < x_len[b], pad_value beyond
 *             (upstream fills -100, :132).  Ties keep the earlier candidate in the order stay, previous cell, skip, as
 *             upstream's strict ">" does.  Too few frames for the labelling is not an error upstream and is not one
 *             here (same walk over -inf cells).  An utterance with invalid lengths or a target outside [0,V) gets a
 *             row of pad_value; so does x_len[b] = 0 (it has no frames).
 *             Rows without a lattice: an empty target (is_ctc = 1, t_len[b] = 0) is `blank` on every frame (upstream's
 *             zeros: its blank is 0).  One frame (x_len[b] = 1) and t_len[b] >= 1 is targets[b,0] whatever t_len[b] is --
 *             upstream's quirk, kept; one frame and no target is `blank`.  is_ctc = 0 with t_len[b] = 0 is 0 on every
 *             frame (upstream would index targets[0]; there is no blank to fall back on).
 *   Smax      the width of `targets`.  The lattice of the widest possible target (2 Smax + 1 cells, is_ctc = 0: Smax)
 *             has to fit a workgroup's 160 KiB of LDS, whatever t_len holds: is_ctc = 1: Smax <= 3172; is_ctc = 0:
 *             Smax <= 6345.  Beyond that: E2E_ERR_UNSUPPORTED before any launch, e2e_last_error() names both numbers,
 *             `out` is untouched.  Utterances of one batch may be swept in different forms (a lattice of at most 512
 *             cells two cells per thread, a wider one in strides of 256): the result does not depend on the form.
 *   workspace >= e2e_ctc_align_workspace_bytes(...): one back-pointer byte per lattice cell and frame
 */
size_t e2e_ctc_align_workspace_bytes(int B, int T, int V, int Smax, int is_ctc);

int e2e_ctc_align(const void* lp, int dtype, int64_t sB, int64_t sT, int64_t sV,
                  const int64_t* targets, int64_t tgt_stride,
                  const int64_t* x_len, const int64_t* t_len,
                  int B, int T, int V, int Smax, int blank, int is_ctc,
                  int64_t* out, int64_t pad_value,
                  void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Word-segmented CTC: plan, gather, finish (additive, ABI 4: nothing above changes meaning).
 * Replaces the host loops of pytorch_end2end/modules/ctc_loss_segmented.py:43-146 (CTCLossSegmented.forward): find the
 * words the model already recognises frame for frame, cut every utterance at the spaces around them, train each piece with
 * its own CTC loss.  The alignment comes from e2e_ctc_align and the pieces' losses from e2e_ctc_loss_fwd_bwd; these three
 * calls are what lies between.  They are asynchronous on `stream`, allocate nothing, never synchronise and are capturable;
 * every argument error the host can see is E2E_ERR_ARG before any launch.
 *
 * DEFINITION.  Per utterance, n = x_len[b]; a[t] = align[b,t] (e2e_ctc_align on log_softmax(x), is_ctc = 1); p[t] the
 * arg-max column of x[b,t,:], first maximum, NaN counts as the maximum (as e2e_ctc_greedy).
 *   boundaries  State bounds = [0], start_space = -1, clean = 1, wl = 0, last = -1, last_blank = 0.  For t = 0 .. n-1:
 *                 a[t] != p[t]      clean = 0, nothing else changes;
 *                 a[t] == space     if clean and wl >= min_word_length: append start_space if start_space != -1 and
 *                                   bounds[-1] != start_space; append t if t > 0.  In every case start_space = t,
 *                                   clean = 1, wl = 0, last = -1, last_blank = 0;
 *                 a[t] == blank     last_blank = 1 (the space test comes first);
 *                 else              wl += 1 if last_blank or a[t] != last; last = a[t], last_blank = 0.
 *               After the loop n-1 is appended if bounds[-1] != n-1.
 *   segments    len(bounds) <= 2, lengths outside 1 <= x_len <= T, 0 <= t_len <= Smax, or a target outside [0,V): ONE
 *               WHOLE segment, frames 0 .. n-1 with the caller's targets and lengths (out of range: the loss gives it
 *               its NaN slab).  Otherwise for k, start in enumerate(bounds[:-1]): if start != 0 a FRAME segment, the
 *               single frame `start` with the target [a[start]], and start += 1; end = bounds[k+1], minus 1 unless k is
 *               the last; if end >= start a CHUNK, frames start .. end, whose target is a[start..end] with runs collapsed
 *               and blanks dropped afterwards (a a _ a gives a a).  The segments partition the frames 0 .. n-1.
 *               (Upstream counts the segments before it builds them and raises where the two disagree -- a qualifying
 *               space on the last frame, a first boundary at frame 1; here the built list is the definition.)
 *
 * PLAN.
 *   x           (B,T,V) raw logits, strides sB,sT,sV (any), E2E_F32 or E2E_F64
 *   align       (B,T) int64 contiguous
 *   targets, tgt_stride, x_len, t_len, Smax   as for e2e_ctc_loss_fwd_bwd
 *   blank, space  in [0,V); min_word_length any int (<= 0: every clean space qualifies)
 *   table       int32, e2e_ctc_wordseg_table_elems(B,T) = 16 + (B+1) + 5*B*T elements, written:
 *                 [0] N segments  [1] whole  [2] frame  [3] chunk segments  [4] the longest whole / chunk segment in
 *                 frames  [5] its longest target  [6] utterances that were cut  [7..15] 0
 *                 [16 .. 16+B]  first segment of every utterance, and N behind them
 *                 then five arrays of B*T entries, the first N used, utterance-major and in the order above: length in
 *                 frames, target length, kind (E2E_WORDSEG_*), utterance, start frame.
 *               At most sum(x_len) <= B*T segments exist.  Counting is deterministic: per-utterance counts, then a scan.
 *   pool        (B,T) int64: the target of a chunk or frame segment that starts at frame s of utterance b is
 *               pool[b, s .. s + target length) -- a chunk has at most as many labels as frames
 *   workspace   >= e2e_ctc_wordseg_workspace_bytes(B,T), 26 bytes per frame.  It carries the plan's per-frame state to
 *               the gather and finish calls of the same batch: nothing else may write it in between.
 *
 * GATHER.  For the n_idx table indices in idx (device; whole segments and chunks -- frame segments are never gathered; an
 * index outside [0,N) gives an empty row) writes the dense zero-padded batch e2e_ctc_loss_fwd_bwd takes:
 *   xg (n_idx,L,V) contiguous, x's dtype;  tg (n_idx,S) int64;  xlg, tlg (n_idx) int64
 *   L, S        >= the longest listed segment / target (1 <= L <= T, S >= 1); longer ones are cut, which the host avoids
 * A whole segment hands on the caller's own lengths and targets.
 *
 * FINISH.  Called once per gathered batch and a last time with last = 1 (n_idx = 0 allowed):
 *   g_grads (n_idx,L,V), g_losses (n_idx)   what the loss returned for the batch gathered with g_idx, L; x's dtype
 *   grads       (B,T,V) contiguous: every listed segment's rows are copied to its own frames (plain stores; the frames
 *               are disjoint)
 *   last        != 0: also writes the frames no gathered segment owns -- a frame segment in closed form in f64, loss
 *               logsumexp(x_t) - x_t[c], gradient softmax(x_t) - onehot(c); frames t >= x_len[b] 0 (the rest of the NaN
 *               slab for an utterance that is one segment with a loss that is not finite) -- and
 *   losses      (B) x's dtype: the f64 sum of the utterance's segment losses in table order, so that two calls on the
 *               same input agree bit for bit; +inf and NaN propagate per utterance.
 */
#define E2E_WORDSEG_HEADER 16
#define E2E_WORDSEG_WHOLE 0
#define E2E_WORDSEG_FRAME 1
#define E2E_WORDSEG_CHUNK 2

size_t e2e_ctc_wordseg_table_elems(int B, int T);
size_t e2e_ctc_wordseg_workspace_bytes(int B, int T);

int e2e_ctc_wordseg_plan(const void* x, int dtype, int64_t sB, int64_t sT, int64_t sV,
                         const int64_t* align, const int64_t* targets, int64_t tgt_stride,
                         const int64_t* x_len, const int64_t* t_len,
                         int B, int T, int V, int Smax, int blank, int space, int min_word_length,
                         int32_t* table, size_t table_elems, int64_t* pool,
                         void* workspace, size_t workspace_bytes, void* stream);

int e2e_ctc_wordseg_gather(const void* x, int dtype, int64_t sB, int64_t sT, int64_t sV,
                           const int64_t* targets, int64_t tgt_stride,
                           const int64_t* x_len, const int64_t* t_len,
                           int B, int T, int V, int Smax,
                           const int32_t* table, const int64_t* pool,
                           const int32_t* idx, int n_idx, int L, int S,
                           void* xg, int64_t* tg, int64_t* xlg, int64_t* tlg, void* stream);

int e2e_ctc_wordseg_finish(const void* x, int dtype, int64_t sB, int64_t sT, int64_t sV,
                           const int64_t* align, int B, int T, int V, const int32_t* table,
                           const void* g_grads, const void* g_losses, const int32_t* g_idx, int n_idx, int L,
                           int last, void* losses, void* grads,
                           void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* E2E_CTC_H */
