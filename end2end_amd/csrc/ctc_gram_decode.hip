// Gram-CTC decoding (the definition: include/e2e_ctc.h, beside the Gram-CTC loss).
//
// Greedy: the arg-max / collapse kernel of ctc_greedy.hip with blank 0 gives the collapsed columns; gram_expand_kernel
// turns them into base ids (a prefix sum of the grams' lengths over the columns, then a scatter).
//
// Beam search: one workgroup per utterance.  The beam's members (up to 128 prefixes, each with its max_order + 1 slots)
// live in LDS, double buffered.  A frame's candidates meet in an open-addressing table of 64-bit prefix keys in the
// workspace: every member and every (member, column) pair with a non-zero share claims or finds its key with a 64-bit
// compare-and-swap and pushes its own id on the entry's list with an exchange.  Nothing is added there: a share is a
// function of the pair (src * y[c]) and is recomputed by whoever walks the list.  A (prefix, slot) receives at most its
// stay share and one extension share, so a slot is the sum of two numbers and a total the sum of the slots in the order
// 0 .. max_order -- the same bits whatever order the pairs arrived in.  The per-frame cut first drops what cannot matter
// (a full beam's members are W candidates themselves: nothing below the least of their new totals survives); the select
// and the ranking are beam_cut.h's, the select on the bits of the totals (positive doubles order as integers), and the
// survivors become the next members in the order of their ranks.  The table is cleared entry by entry from the frame's
// candidate list.  The read-out walks the (parent node, column) pool backwards and expands the grams.
//
// With a word language model (e2e_gram_ctc_beam_nbest_lm, the LM instance): a member also carries the LM fields of
// asg_beam.hip's members, in LDS beside the slots.  They are functions of the base-id sequence alone, so a candidate may take
// them from any pair that spells it: walk_gram applies get_next_prefix's rule to the gram's ids one at a time and asks the
// model only where the answer can matter (a word's last id inside the gram, the gram's last id).  The model is not asked
// per pair and frame: when a prefix becomes a member the answers of its V children (lm_score, num_words, num_oov) are
// computed once and kept in a row of the workspace for as long as the prefix stays in the beam (2 W rows, a member keeps its
// row's index).  The cut then runs on okey(log tot + lmwt lm - wip words + oov_penalty oovs) as the ASG
// kernel's does.  The no-LM instance is the kernel as it was, instruction for instruction (tools/diag/isa_compare.py).
//
// Restricted to the model's lexicon, and with label timestamps (e2e_gram_ctc_beam_nbest_opt, the LEX and TS instances): the
// rule of the header is applied per base id, which walk_gram<LEX> decides at the places where it asks the model anyway; a
// member's answer row also says which of its children exist, and a pair without a child is dropped before it claims a table
// entry, so an inadmissible sequence never has one.  The timesteps are read off the nodes' numbers in the read-out.
//
// Fed in chunks (e2e_gram_ctc_beam_stream, the ST instances): between two frames the search is one Members set, with the LM
// fields one LmMembers set, n_mem, esum, the overflow flag and the node pool -- that is an utterance's state row, which the
// caller owns (header | Members | LmMembers | nodes).  The candidate table is empty between frames, the pair buffers are a
// frame's scratch, and the answer cache is refilled at resume from the members' own sequences (rows 0 .. n_mem - 1), as the
// per-frame refill fills a new member's row.  Node numbers count the frames of the stream.  DESIGN.md 4.7, Streaming.
//
// The beam search's kernel and the host-side helpers are in ctc_gram_decode.h: ctc_gram_decode_cut.hip instantiates the same
// kernel with CUT (per-frame label pruning) in an object of its own.  Here: the greedy kernel and the unpruned entries.
#include "ctc_gram_decode.h"

namespace e2e {

int launch_greedy(const void* x, int dtype, int64_t sB, int64_t sT, int64_t sV, const int64_t* x_len,
                  int B, int T, int V, int blank, int64_t* out, int64_t* out_len, hipStream_t stream);

namespace {

constexpr int kExpandThreads = 256;

// ---- greedy: columns -> base ids ----------------------------------------------------------------------------------
struct GramExpandParams {
  const int64_t* cols; const int64_t* cols_len; const int32_t* gram_ids; const int32_t* gram_len;
  int T, V, K; int64_t* out; int64_t* out_len;
};

__global__ __launch_bounds__(kExpandThreads) void gram_expand_kernel(GramExpandParams p) {
  __shared__ int wave_tot[kExpandThreads / 64];
  __shared__ int carry;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int64_t* cols = p.cols + (int64_t)b * p.T;
  const int64_t width = (int64_t)p.T * p.K;
  int64_t* out = p.out + (int64_t)b * width;
  const int64_t nq = p.cols_len[b];
  const int n = nq < 0 ? 0 : (nq > p.T ? p.T : (int)nq);
  if (tid == 0) carry = 0;
  __syncthreads();
  for (int i0 = 0; i0 < n; i0 += kExpandThreads) {
    const int i = i0 + tid;
    int c = 0, len = 0;
    if (i < n) {
      const int64_t cq = cols[i];
      c = (cq >= 1 && cq < p.V) ? (int)cq : 0;
      len = c ? order_of(p.gram_len, c, p.K) : 0;
    }
    int incl = len;
    for (int o = 1; o < 64; o <<= 1) { const int v = __shfl_up(incl, o, 64); if (lane >= o) incl += v; }
    if (lane == 63) wave_tot[wid] = incl;
    __syncthreads();
    int base = carry + incl - len, total = 0;
    for (int w = 0; w < kExpandThreads / 64; w++) { if (w < wid) base += wave_tot[w]; total += wave_tot[w]; }
    for (int j = 0; j < len; j++) out[base + j] = (int64_t)p.gram_ids[c * kMaxK + j];
    __syncthreads();
    if (tid == 0) carry += total;
    __syncthreads();
  }
  const int total = carry;
  for (int64_t i = total + tid; i < width; i += kExpandThreads) out[i] = 0;
  if (tid == 0) p.out_len[b] = total;
}

}  // namespace
}  // namespace e2e

using namespace e2e;

extern "C" {

int e2e_gram_ctc_greedy(const void* x, int dtype, int64_t sB, int64_t sT, int64_t sV, const int64_t* x_len,
                        int B, int T, int V, const int32_t* gram_ids, const int32_t* gram_len, int max_order,
                        int64_t* out, int64_t* out_len, int64_t* cols, int64_t* cols_len, void* stream) {
  if (dtype != E2E_F32 && dtype != E2E_F64 && !dtype_is_16bit(dtype)) { set_error("dtype must be E2E_F32, E2E_F64, E2E_F16 or E2E_BF16"); return E2E_ERR_ARG; }
  if (B < 0 || T < 1 || V < 1) { set_error("bad sizes B=%d T=%d V=%d", B, T, V); return E2E_ERR_ARG; }
  if (max_order < 1 || max_order > kMaxK) { set_error("max_order %d is not in [1, %d]", max_order, kMaxK); return E2E_ERR_ARG; }
  if ((int64_t)T * max_order > 0x7fffffffLL) { set_error("T * max_order = %lld does not fit", (long long)T * max_order); return E2E_ERR_UNSUPPORTED; }
  if (B > 0 && (!x || !x_len || !gram_ids || !gram_len || !out || !out_len || !cols || !cols_len)) { set_error("null pointer argument"); return E2E_ERR_ARG; }
  if (B == 0) return E2E_OK;
  const int rc = launch_greedy(x, dtype, sB, sT, sV, x_len, B, T, V, 0, cols, cols_len, (hipStream_t)stream);
  if (rc != E2E_OK) return rc;
  GramExpandParams p{cols, cols_len, gram_ids, gram_len, T, V, max_order, out, out_len};
  hipLaunchKernelGGL(gram_expand_kernel, dim3(B), dim3(kExpandThreads), 0, (hipStream_t)stream, p);
  E2E_HIP_CHECK(hipGetLastError(), "gram_expand_kernel launch");
  return E2E_OK;
}

int e2e_gram_beam_max_width(int V, int max_order) {
  if (V < 1 || max_order < 1 || max_order > kMaxK) return 0;
  const int w = kMaxPairs / V;
  return w < kMaxW ? w : kMaxW;
}

size_t e2e_gram_beam_workspace_bytes(int B, int T, int V, int max_order, int beam_width) {
  return e2e_gram_beam_workspace_bytes_lm(B, T, V, max_order, beam_width, 0);
}

int e2e_gram_ctc_beam_nbest(const void* lp, int dtype, int64_t sB, int64_t sT, int64_t sV, const int64_t* x_len,
                            int B, int T, int V, const int32_t* gram_ids, const int32_t* gram_len, int max_order,
                            int beam_width, int nbest, int64_t* out, int64_t max_out, int64_t* out_len, int64_t* n_hyp,
                            double* scores, void* workspace, size_t workspace_bytes, void* stream) {
  if (const int rc = check_beam_args(dtype, B, T, V, max_order, beam_width, nbest, max_out)) return rc;
  BeamLayout L;
  if (!beam_layout(T, V, max_order, beam_width, L)) { set_error("T=%d frames are more than the search takes", T); return E2E_ERR_UNSUPPORTED; }
  if (const int rc = check_pointers(B, {lp, x_len, gram_ids, gram_len, out_len, n_hyp, scores, max_out > 0 ? out : unused})) return rc;
  if (B == 0) return E2E_OK;
  if (const int rc = check_workspace(workspace, workspace_bytes, (size_t)B * L.per_utt, "e2e_gram_beam_workspace_bytes")) return rc;
  GramBeamParams p;
  fill_params(p, lp, dtype, sB, sT, sV, x_len, B, T, V, gram_ids, gram_len, max_order, beam_width, nbest, out, max_out, out_len,
              n_hyp, scores, workspace, L, L.per_utt, L.off_nodes);
  hipLaunchKernelGGL(gram_beam_kernel<false>, dim3(B), dim3(kBeamThreads), 0, (hipStream_t)stream, p);
  E2E_HIP_CHECK(hipGetLastError(), "gram_beam_kernel launch");
  return E2E_OK;
}

size_t e2e_gram_beam_workspace_bytes_lm(int B, int T, int V, int max_order, int beam_width, int with_lm) {
  BeamLayout L;
  if (B < 0 || !beam_layout(T, V, max_order, beam_width, L, with_lm != 0)) return 0;
  return (size_t)B * L.per_utt + 256;
}

int e2e_gram_ctc_beam_nbest_opt(const void* lp, int dtype, int64_t sB, int64_t sT, int64_t sV, const int64_t* x_len,
                                int B, int T, int V, const int32_t* gram_ids, const int32_t* gram_len, int max_order,
                                int num_base_labels, int beam_width, int space_id, const e2e_lm* lm, double lmwt,
                                double wip, double oov_penalty, int nbest, int64_t* out, int64_t max_out, int64_t* out_len,
                                int64_t* n_hyp, double* scores, int32_t* counts, void* workspace, size_t workspace_bytes,
                                void* stream, const e2e_gram_beam_opts* opts) {
  const bool restricted = opts && opts->restrict_to_lexicon != 0;
  int64_t* timesteps = opts ? opts->timesteps : nullptr;
  if (const int rc = check_beam_args(dtype, B, T, V, max_order, beam_width, nbest, max_out)) return rc;
  if (const int rc = check_scored_args(V, num_base_labels, space_id, lm, restricted)) return rc;
  BeamLayout L;
  if (!beam_layout(T, V, max_order, beam_width, L, lm != nullptr)) { set_error("T=%d frames are more than the search takes", T); return E2E_ERR_UNSUPPORTED; }
  if (const int rc = check_pointers(B, {lp, x_len, gram_ids, gram_len, out_len, n_hyp, scores, counts, max_out > 0 ? out : unused})) return rc;
  if (B == 0) return E2E_OK;
  if (const int rc = check_model_device(lm)) return rc;
  if (const int rc = check_workspace(workspace, workspace_bytes, (size_t)B * L.per_utt, "e2e_gram_beam_workspace_bytes_lm")) return rc;
  GramOptParams o;
  GramLmParams& q = o.l;
  fill_params(q.b, lp, dtype, sB, sT, sV, x_len, B, T, V, gram_ids, gram_len, max_order, beam_width, nbest, out, max_out, out_len,
              n_hyp, scores, workspace, L, L.per_utt, L.off_nodes);
  fill_lm_params(q, num_base_labels, space_id, lm, lmwt, wip, oov_penalty, counts, L);
  o.timesteps = timesteps;
  hipStream_t s = (hipStream_t)stream;
  // (neither option: the kernel and the parameter block of e2e_gram_ctc_beam_nbest_lm)
  if (!restricted && !timesteps) hipLaunchKernelGGL(gram_beam_kernel<true>, dim3(B), dim3(kBeamThreads), 0, s, q);
  else if (!restricted) hipLaunchKernelGGL((gram_beam_kernel<true, false, true>), dim3(B), dim3(kBeamThreads), 0, s, o);
  else if (!timesteps) hipLaunchKernelGGL((gram_beam_kernel<true, true, false>), dim3(B), dim3(kBeamThreads), 0, s, o);
  else hipLaunchKernelGGL((gram_beam_kernel<true, true, true>), dim3(B), dim3(kBeamThreads), 0, s, o);
  E2E_HIP_CHECK(hipGetLastError(), "gram_beam_kernel (LM) launch");
  return E2E_OK;
}

int e2e_gram_ctc_beam_nbest_lm(const void* lp, int dtype, int64_t sB, int64_t sT, int64_t sV, const int64_t* x_len,
                               int B, int T, int V, const int32_t* gram_ids, const int32_t* gram_len, int max_order,
                               int num_base_labels, int beam_width, int space_id, const e2e_lm* lm, double lmwt,
                               double wip, double oov_penalty, int nbest, int64_t* out, int64_t max_out, int64_t* out_len,
                               int64_t* n_hyp, double* scores, int32_t* counts, void* workspace, size_t workspace_bytes,
                               void* stream) {
  return e2e_gram_ctc_beam_nbest_opt(lp, dtype, sB, sT, sV, x_len, B, T, V, gram_ids, gram_len, max_order, num_base_labels,
                                     beam_width, space_id, lm, lmwt, wip, oov_penalty, nbest, out, max_out, out_len, n_hyp,
                                     scores, counts, workspace, workspace_bytes, stream, nullptr);
}

size_t e2e_gram_beam_stream_row_bytes(int max_frames, int V, int max_order, int beam_width, int scored, int with_lm) {
  StreamLayout S; BeamLayout L;
  return stream_layout(max_frames, V, max_order, beam_width, scored != 0, with_lm != 0, S, L) ? S.total : 0;
}

size_t e2e_gram_beam_stream_workspace_bytes(int B, int V, int max_order, int beam_width, int scored, int with_lm) {
  StreamLayout S; BeamLayout L;
  if (B < 0 || !stream_layout(1, V, max_order, beam_width, scored != 0, with_lm != 0, S, L)) return 0;
  return (size_t)B * S.ws_per_utt + 256;
}

int e2e_gram_ctc_beam_stream(const void* lp, int dtype, int64_t sB, int64_t sT, int64_t sV, const int64_t* chunk_len,
                             int B, int T, int V, const int32_t* gram_ids, const int32_t* gram_len, int max_order,
                             int num_base_labels, int beam_width, int scored, int space_id, const e2e_lm* lm, double lmwt,
                             double wip, double oov_penalty, void* state, size_t row_bytes, int max_frames,
                             int nbest, int64_t* out, int64_t max_out, int64_t* out_len, int64_t* n_hyp, double* scores,
                             int32_t* counts, int64_t* frames_done, void* workspace, size_t workspace_bytes, void* stream,
                             const e2e_gram_beam_opts* opts) {
  const bool sc = scored != 0;
  const bool restricted = sc && opts && opts->restrict_to_lexicon != 0;
  // every argument error the host can see, before any launch
  if (const int rc = check_beam_args(dtype, B, T, V, max_order, beam_width, nbest, nbest > 0 ? max_out : 0, 0)) return rc;
  if (!sc && (lm || counts || opts)) {
    set_error("scored = 0 is the search of e2e_gram_ctc_beam_nbest: lm, counts and opts must be NULL");
    return E2E_ERR_ARG;
  }
  if (sc) { if (const int rc = check_scored_args(V, num_base_labels, space_id, lm, restricted)) return rc; }
  if (max_frames < 1 || max_frames > (1 << 22)) { set_error("max_frames=%d outside [1, %d]", max_frames, 1 << 22); return E2E_ERR_ARG; }
  StreamLayout S; BeamLayout L;
  if (!stream_layout(max_frames, V, max_order, beam_width, sc, lm != nullptr, S, L)) {
    set_error("max_frames=%d frames are more than the search takes", max_frames); return E2E_ERR_UNSUPPORTED;
  }
  if (const int rc = check_row_bytes(row_bytes, S.total, "e2e_gram_beam_stream_row_bytes")) return rc;
  if (const int rc = check_pointers(B, {lp, chunk_len, gram_ids, gram_len, state, frames_done})) return rc;
  if (nbest > 0) if (const int rc = check_pointers(B, {out_len, n_hyp, scores, sc ? counts : unused, max_out > 0 ? out : unused})) return rc;
  if (const int rc = check_state_aligned(B, state)) return rc;
  if (B == 0) return E2E_OK;
  if (const int rc = check_workspace(workspace, workspace_bytes, (size_t)B * S.ws_per_utt, "e2e_gram_beam_stream_workspace_bytes")) return rc;
  if (const int rc = check_model_device(lm)) return rc;
  GramStreamParams sp;
  memset(&sp, 0, sizeof(sp));
  GramLmParams& q = sp.o.l;
  fill_params(q.b, lp, dtype, sB, sT, sV, chunk_len, B, T, V, gram_ids, gram_len, max_order, beam_width, nbest, out,
              nbest > 0 ? max_out : 0, out_len, n_hyp, scores, workspace, L, S.ws_per_utt, 0);     // (the nodes are the row's)
  fill_lm_params(q, num_base_labels, space_id, lm, lmwt, wip, oov_penalty, counts, L);
  sp.o.timesteps = sc && nbest > 0 && opts ? opts->timesteps : nullptr;
  GramStream& s = sp.s;
  s.rows = reinterpret_cast<unsigned char*>(state); s.row_bytes = row_bytes; s.off_lm = S.off_lm; s.off_nodes = S.off_nodes;
  s.frames_done = frames_done;
  s.cfg.magic = kGramStreamMagic; s.cfg.V = V; s.cfg.K = max_order; s.cfg.R = sc ? num_base_labels : 0; s.cfg.W = beam_width;
  s.cfg.scored = sc ? 1 : 0; s.cfg.has_lm = lm ? 1 : 0; s.cfg.restricted = restricted ? 1 : 0; s.cfg.max_frames = max_frames;
  hipStream_t hs = (hipStream_t)stream;
  if (!sc) hipLaunchKernelGGL((gram_beam_kernel<false, false, false, true>), dim3(B), dim3(kBeamThreads), 0, hs, sp);
  else if (!restricted) hipLaunchKernelGGL((gram_beam_kernel<true, false, false, true>), dim3(B), dim3(kBeamThreads), 0, hs, sp);
  else hipLaunchKernelGGL((gram_beam_kernel<true, true, false, true>), dim3(B), dim3(kBeamThreads), 0, hs, sp);
  E2E_HIP_CHECK(hipGetLastError(), "gram_beam_kernel (stream) launch");
  return E2E_OK;
}

}  // extern "C"
