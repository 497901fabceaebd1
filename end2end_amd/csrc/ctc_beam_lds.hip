// The prefix beam search's kernel that keeps the beam in LDS (ctc_beam_common.h has the algorithm and the shared phases).
// Compiled once per input dtype, -DE2E_BEAM_IO=float | double | e2e::f16_t | e2e::bf16_t: ctc_beam_lds.f32.o, .f64.o, .f16.o,
// .bf16.o, each with the 9 LM kinds x (streaming or not) = 18 instances of that dtype and lds_kernel<IO> to hand them out.
// The instrumented build (E2E_BEAM_PROFILE) defines its counters and their readers here, beside the kernels that write them,
// and is given to the f32 object alone (tools/diag/build_profile_lib.sh).
#include <utility>

#include "ctc_beam_common.h"

#ifdef E2E_BEAM_PROFILE
__device__ unsigned long long g_beam_prof[16];
__device__ unsigned long long g_beam_sigs[1 << 17];
__device__ int g_beam_nsig;
#define BPROF(slot) do { if (b == 0 && tid == 0) { const unsigned long long _n = __builtin_amdgcn_s_memtime(); g_beam_prof[slot] += _n - _tprev; _tprev = _n; } } while (0)
#else
#define BPROF(slot) do {} while (0)
#endif

namespace e2e {
namespace beamk {
namespace {      // (the kernels have internal linkage: only the table below names them)

// ST: the streaming call's instance.  The resume and suspend phases are compiled into it alone, so the kernels of the calls that
// decode whole utterances are instruction for instruction what they are without them (as one kernel with a test on a null
// pointer, the phases cost every instance ~30 more spilled SGPRs and the fast LM instance two VGPRs spilled to scratch).
template <typename IO, int LMK, bool ST>
__global__ __launch_bounds__(kThreads) void ctc_beam_kernel(BeamParams p) {
  constexpr bool LM = LMK != 0, RS = lmk_restricted(LMK);
  extern __shared__ __align__(16) unsigned char smem[];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int V = p.V, W = p.W, blank = p.blank;
  // ---- LDS carve-up ----
  unsigned char* q8 = smem;
  double* key = (double*)q8; q8 += sizeof(double) * p.CMAX;          // score of candidate d: old members, then the n*V pairs
  double* srow2 = (double*)q8; q8 += sizeof(double) * 2 * V;         // this step's and the next step's log-probabilities
  double* skey = (double*)q8; q8 += sizeof(double) * (p.WP2 + kSelSmall);   // the gathered candidates, for the final ordering
  // (the two member sets and the two slot maps are addressed as "base + set * size", never through an array of
  // pointer structs: a pointer that went through memory loses its LDS address space and every access through it
  // becomes a FLAT instruction -- slower, and not ordered by an LDS-only barrier)
  unsigned char* const mem0 = q8;
  const size_t mbytes = Members::bytes(W);
  q8 += 2 * mbytes;
  Members M0; M0.carve(mem0, W);
  int* sidx = (int*)q8; q8 += sizeof(int) * (p.WP2 + kSelSmall);
  int* const ctab0 = (int*)q8; q8 += sizeof(int) * 2 * (size_t)W * V; // [set][member][V] child tables (weak next_data)
  int* hist = (int*)q8; q8 += sizeof(int) * 2 * kSelBins;
  int* s_part = (int*)q8; q8 += sizeof(int) * 64;
  int* const sm0 = (int*)q8; q8 += sizeof(int) * 4 * p.HS;            // [set][key | val][HS]
  LmAnswer* const lmc0 = (LmAnswer*)q8; if (LM) q8 += 2 * sizeof(LmAnswer) * (size_t)W * V;   // [set][member][V] the LM's answers
  int* const lab_off = (int*)q8; if (LM) q8 += sizeof(int) * (size_t)(V + 2);
  unsigned char* const lab_bytes = q8; if (LM) q8 += kLabelLdsBytes;
  int* const lab_one = (int*)q8; if (LM) q8 += sizeof(int) * (size_t)V;
  LabelTab lt; lt.off = p.lm.label_off; lt.bytes = p.lm.label_bytes; lt.one = nullptr;
  auto slot_map = [&](int set) { SlotMap m; m.key = sm0 + set * 2 * p.HS; m.val = m.key + p.HS; m.mask = p.HS - 1; return m; };
  __shared__ int s_next_node, s_err, s_krem, s_done, s_bin;
  // per-step accumulators, double-buffered by step parity: a step resets the NEXT step's set while nobody uses it, so
  // that no barrier is needed between the end of one step and the pair loop of the next
  __shared__ int s_total_new2[2], s_nnew2[2];
  __shared__ unsigned s_hi2[2], s_lo2[2];
  __shared__ unsigned long long s_prefix;

  // (streaming: the utterance's state row holds the node pool and the nodes' frames; null, at compile time, in every other call)
  unsigned char* const st_row = ST ? p.st_rows + (size_t)b * p.st_row_bytes : nullptr;
  BeamNode* nodes = ST ? reinterpret_cast<BeamNode*>(st_row + p.st_nodes_off) : p.nodes + (size_t)b * p.NCAP;
  int* const node_t = ST ? (p.st_ts_off ? reinterpret_cast<int*>(st_row + p.st_ts_off) : nullptr)
                         : p.node_t ? p.node_t + (size_t)b * p.NCAP : nullptr;         // (uniform: null in the plain call)
  const IO* lp = reinterpret_cast<const IO*>(p.lp) + (int64_t)b * p.sB;
  int64_t Tq = p.x_len[b];
  const int T = Tq < 0 ? 0 : (Tq > p.T ? p.T : (int)Tq);
  // frames consumed before this call (node_t holds global frames; everything keyed on step parity uses the local step)
  int t0 = 0, n0 = 1;
  bool resume = false;
  if (ST) {
    t0 = stream_open(p, st_row, T, resume);
    if (t0 < 0) { stream_refuse(p, t0); return; }
    if (resume) n0 = __builtin_amdgcn_readfirstlane(reinterpret_cast<const StreamHeader*>(st_row)->n);
  }

  // ---- pools, root prefix (get_initial_prefix, :222-230) ----
  for (int c = tid; c < n0 * V; c += kThreads) ctab0[c] = -1;                        // set 0: member 0 = the root, or the resumed members
  for (int h = tid; h < p.HS; h += kThreads) { sm0[h] = -1; sm0[2 * p.HS + h] = -1; }
  if (T > 0) for (int c = tid; c < V; c += kThreads) srow2[c] = (double)lp[(int64_t)c * p.sV];
  if (LM) {
    const int nbytes = p.lm.label_off[V];
    if (nbytes <= kLabelLdsBytes) {                       // (uniform) the spellings fit: read them from LDS from now on
      for (int c = tid; c <= V; c += kThreads) lab_off[c] = p.lm.label_off[c];
      for (int i = tid; i < nbytes; i += kThreads) lab_bytes[i] = p.lm.label_bytes[i];
      lt.off = lab_off; lt.bytes = lab_bytes;
    }
    for (int c = tid; c < V; c += kThreads) {
      const int o0 = p.lm.label_off[c];
      int ch = -1;
      if (p.lm.label_off[c + 1] == o0 + 1) {
        ch = p.lm.label_bytes[o0];
        if (p.lm.fold_case && ch >= 'A' && ch <= 'Z') ch += 32;
      }
      lab_one[c] = ch;
    }
    lt.one = lab_one;
  }
  if (tid == 0) {
    s_next_node = 1; s_err = 0;                                                     // node 0 is taken
    s_hi2[0] = 0u; s_lo2[0] = 0xffffffffu; s_total_new2[0] = 0; s_nnew2[0] = 0;
    if (!ST || !resume) init_root(p, nodes, M0);
    else s_next_node = reinterpret_cast<const StreamHeader*>(st_row)->next_node;
  }
  if (ST && resume) stream_load_members(mem0, st_row, mbytes);
  __syncthreads();
  if (!ST || !resume) {
    if (tid == 0) slot_map(0).insert(0, 0);
    if (LM) for (int c = tid; c < V; c += kThreads) if (c != blank && c != p.space_id) lmc0[c] = lm_query<lmk_fast(LMK), RS, lmk_hom(LMK)>(p, lt, M0.lm[0], -1, c);
  } else {
    // what a step rebuilds: the slot map, the child tables (one entry per guard, as rebuild_guards writes them) and the
    // members' LM answers (asked as a new member's are: the same function of the member's state)
    const SlotMap map0 = slot_map(0);
    for (int i = tid; i < n0; i += kThreads) {
      map0.insert(M0.node[i], i);
      const int go = M0.gown[i];
      if (go >= 0) ctab0[go * V + M0.gchar[i]] = M0.gnode[i];
    }
    if (LM) for (int e = tid; e < n0 * V; e += kThreads) {
      const int j2 = e / V, c = e - j2 * V;
      if (c != blank && c != p.space_id) lmc0[e] = lm_query<lmk_fast(LMK), RS, lmk_hom(LMK)>(p, lt, M0.lm[j2], M0.last[j2], c);
    }
  }
  __syncthreads();
  int n = n0, cur = 0;
  // the pair loop's thread layout depends on n alone, and n is W for all but an utterance's first steps: worked out when n
  // changes (three integer divisions, ~100 instructions per thread of a phase that is bound by the instructions it issues)
  int lay_n = -1, lay_P = 1, lay_mpp = kThreads, lay_ii0 = 0, lay_part = 0;
  unsigned lay_nmagic = 0u;          // ceil(2^32 / n): q / n for q < W * V by one multiplication (n > 1)
  // e / V for row indices e < W * V <= kMaxCand by multiplication: ceil(2^32 / V), exact while e * V < 2^32
  const unsigned v_magic = V > 1 ? (unsigned)((0x100000000ULL + (unsigned)V - 1u) / (unsigned)V) : 0u;
  auto div_v = [&](int e) -> int { return V > 1 ? (int)__umulhi((unsigned)e, v_magic) : e; };
#ifdef E2E_BEAM_PROFILE
  unsigned long long _tprev = __builtin_amdgcn_s_memtime();
  if (b == 0 && tid == 0) for (int i = 0; i < 16; i++) g_beam_prof[i] = 0;
#endif

  for (int t = 0; t < T; t++) {
    Members A, Bm;
    A.carve(mem0 + (size_t)cur * mbytes, W);
    Bm.carve(mem0 + (size_t)(cur ^ 1) * mbytes, W);
    const SlotMap mapA = slot_map(cur);              // node -> position among the current members
    const SlotMap mapB = slot_map(cur ^ 1);          // ... among the members this step selects (filled in the rebuild)
    unsigned long long* const ukey = reinterpret_cast<unsigned long long*>(key);   // inside the step key[] holds okey(score)
    unsigned long long* const uskey = reinterpret_cast<unsigned long long*>(skey);
    const int* const ctab = ctab0 + (size_t)cur * W * V;          // child tables of the current members: [member][V]
    int* const ctabB = ctab0 + (size_t)(cur ^ 1) * W * V;         // ... of the members this step selects
    const LmAnswer* const lmcA = lmc0 + (size_t)cur * W * V;
    LmAnswer* const lmcB = lmc0 + (size_t)(cur ^ 1) * W * V;
    double* const srow = srow2 + (t & 1) * V;
    // the next step's row is requested now and parked in LDS at the end of the step: no global round trip at a
    // step's start
    double next_lp = 0.0;
    if (tid < V && t + 1 < T) next_lp = (double)lp[(int64_t)(t + 1) * p.sT + (int64_t)tid * p.sV];
    // (no barrier here: a member's inc / kept / full were set when it was placed, this step's accumulators were reset
    // during the previous step, and the next beam's slot map, child tables and the selection's first histogram are
    // cleared during the members phase below)
    const int ps = t & 1;
    unsigned& s_hi = s_hi2[ps]; unsigned& s_lo = s_lo2[ps];
    int& s_total_new = s_total_new2[ps]; int& s_nnew = s_nnew2[ps];
    // pairs: candidate q = c*n + i is the reference's order (character outer, prefix inner, :370-395).  The threads are
    // laid out member-major -- P threads per member, each taking every P-th character -- so that what a pair needs of
    // its member (probabilities, last character, word count, LM state) is read once per thread, not once per pair.
    const int npairs = n * V;
    if (n != lay_n) {                                           // (uniform)
      lay_n = n; lay_P = n < kThreads ? kThreads / n : 1; lay_mpp = kThreads / lay_P; lay_ii0 = tid / lay_P; lay_part = tid - lay_ii0 * lay_P;
      lay_nmagic = n > 1 ? (unsigned)((0x100000000ULL + (unsigned)n - 1u) / (unsigned)n) : 0u;
    }
    const int P = lay_P;                                        // threads per member
    const int members_per_pass = lay_mpp;
    const int part = lay_part;
    int my_new = 0;
    // blank shares, child shares, scores of the would-be prefixes (weak child lookup, :250-252)
    // (the high words of the largest key of all and of the smallest key of the old members bracket the selection
    // threshold; they are collected while the keys are produced)
    unsigned key_hi = 0u, key_lo = 0xffffffffu;
    for (int ii = lay_ii0; ii < n; ii += members_per_pass) {
      const double full = A.full[ii], ppb = A.ppb[ii];
      const int last = A.last[ii];
      const LmFields pr = score_fields<LM>(A.lm[ii]);
      for (int ci = part; ci < V; ci += P) {
        const double curp = srow[ci];
        unsigned long long* const slot = ukey + n + ci * n + ii;
        if (ci == blank) { *slot = kNoCandKey; A.npb[ii] = curp + full; continue; }   // :374-376 (prob_blank was -inf)
        const double val = curp + (ci == last ? ppb : full);                     // :383-385 / :389-391
        const int k = ctab[ii * V + ci];
        unsigned long long uk = kNoCandKey;
        if (k >= 0) {
          const int j = mapA.find(k);
          if (j >= 0) A.inc[j] = val;            // the child is a beam member: its share from this parent
          // else: alive but pruned (Q7) -- the probability is lost and the slot stays taken
        } else {
          const LmAnswer ans = answer_at<LM>(lmcA, ii * V + ci);
          if (!RS || !lexicon_forbids(p, pr, last, ci, ans)) {   // (forbidden: no child, no candidate; the member's own
            uk = child_key<LM>(p, pr, last, ci, ans, val);       //  repeated-character share is update_members' either way)
            key_hi = max(key_hi, (unsigned)(uk >> 32));
            my_new++;
          }
        }
        *slot = uk;
      }
    }
    {
      const int incl = wave_scan_i(my_new);
      if (lane == 63 && incl) atomicAdd(&s_total_new, incl);
    }
    key_hi = (unsigned)wave_max_i((int)(key_hi ^ 0x80000000u)) ^ 0x80000000u;     // (signed max on biased values)
    if (lane == 0) atomicMax(&s_hi, key_hi);
    lds_barrier();
    BPROF(1);
    update_members<LM>(p, A, n, [&](int c) { return srow[c]; }, ukey, key_hi, key_lo);
    if (wid < (n + 63) / 64) {
      key_hi = (unsigned)wave_max_i((int)(key_hi ^ 0x80000000u)) ^ 0x80000000u;
      key_lo = ~((unsigned)wave_max_i((int)((~key_lo) ^ 0x80000000u)) ^ 0x80000000u);
      if (lane == 0) { atomicMax(&s_hi, key_hi); atomicMin(&s_lo, key_lo); }
    }
    {
      // housekeeping for the phases that follow, by the waves without members (all waves if every wave has some): the
      // member update above is two dependent f64 log-sum-exps on two waves, the other fourteen would only wait
      const int mw = (n + 63) >> 6, nw = kThreads / 64;
      const int ctid = mw < nw ? tid - 64 * mw : tid, cstride = 64 * (mw < nw ? nw - mw : nw);
      if (ctid == 0) { s_hi2[ps ^ 1] = 0u; s_lo2[ps ^ 1] = 0xffffffffu; s_total_new2[ps ^ 1] = 0; s_nnew2[ps ^ 1] = 0; }
      if (ctid >= 0) {
        for (int h = ctid; h < p.HS; h += cstride) mapB.key[h] = -1;
        for (int e = ctid; e < W * V; e += cstride) ctabB[e] = -1;
        for (int h = ctid; h < kSelBins; h += cstride) hist[h] = 0;      // (the second histogram is cleared by the pass before it)
      }
    }
    lds_barrier();
    BPROF(2);
    const int total_new = s_total_new;
    const int nreal = n + total_new;                // candidates that exist
    const int ntot = n + npairs;                    // entries of key[]
    const int nsel = nreal > W ? W : nreal;
    int* const sel = hist + kSelBins;               // (no pruning only) the candidates in beam order
    // (LM: scratch of the answer phase, in regions that are dead by then -- the first histogram, the gathered candidates,
    // the candidate keys)
    int* const newlist = sidx;                                                        // new members that have to ask
    int* const ldr = reinterpret_cast<int*>(skey);                                    // leader of member j
    unsigned long long* const tsig = reinterpret_cast<unsigned long long*>(hist);     // open addressing: signature -> smallest rank
    // candidate d takes place j of the new beam (the other member set): a member that stays is copied, a pair becomes a
    // prefix -- node, LM state, its own guard.  Called by the thread that has just worked out the candidate's rank.
    // ... in two halves that touch different fields of the new member: what the lattice needs (probabilities, node, guard,
    // slot map) and the LM state -- with a language model they run on different waves (below).
    auto place_core = [&](int j, int d) {
      if (d < n) {
        const int i = d;
        A.kept[i] = 1; A.newpos[i] = j; Bm.from[j] = i;
        Bm.ppb[j] = A.npb[i]; Bm.ppnb[j] = A.npnb[i]; Bm.full[j] = A.nfull[i];
        Bm.node[j] = A.node[i]; Bm.last[j] = A.last[i];
        Bm.gown[j] = A.gown[i]; Bm.gchar[j] = A.gchar[i]; Bm.gnode[j] = A.gnode[i];     // (owner: position in A, for now)
        mapB.insert(A.node[i], j);
      } else {
        const int q = d - n;
        const int c = n > 1 ? (int)__umulhi((unsigned)q, lay_nmagic) : q, i = q - c * n;      // (q / n: exact for q * n < 2^32)
        const double val = srow[c] + (c == A.last[i] ? A.ppb[i] : A.full[i]);
        int k = atomicAdd(&s_next_node, 1);                                       // make_shared<Prefix>, :254
        if (k >= p.NCAP) { s_err = 1; k = 0; }
        else {
          BeamNode nn;
          nn.parent = A.node[i]; nn.last_char = c;
          nodes[k] = nn;                                                          // (fire and forget)
          if (node_t) node_t[k] = ST ? t0 + t : t;
          mapB.insert(k, j);
        }
        Bm.ppb[j] = ninf(); Bm.ppnb[j] = val; Bm.full[j] = lse2(val, ninf()); Bm.node[j] = k; Bm.last[j] = c;
        Bm.gown[j] = i; Bm.gchar[j] = c; Bm.gnode[j] = k;                         // its own guard, if its parent stays
        Bm.from[j] = -1;
      }
    };
    auto place_lm = [&](int j, int d) {
      if (d < n) {
        copy_lm<LM>(Bm.lm[j], A.lm[d]);
      } else {
        const int q = d - n;
        const int c = n > 1 ? (int)__umulhi((unsigned)q, lay_nmagic) : q, i = q - c * n;
        child_lm<LM>(p, lt, A.lm[i], A.last[i], c, answer_at<LM>(lmcA, i * V + c), Bm.lm[j]);                 // (straight into LDS: a local LmFields lives in scratch)
      }
    };
    auto place = [&](int j, int d) { place_core(j, d); place_lm(j, d); };
    // The members are built by W threads on two waves, not by the ranking threads (one lane in eight of all sixteen waves:
    // every wave walked the whole of place() -- with a language model some 400 instructions -- for eight useful lanes,
    // and the phase was bound by the instructions the four SIMDs had to issue).  (Called at the end of both branches
    // below: behind their join it would cost the LM instances two VGPRs spilled to scratch.)
    auto place_all = [&]() {
      lds_barrier();
      if (LM) {
        // blocks of 128 threads alternate between the two halves: waves 0-1 the lattice half of members 0..127, waves 2-3
        // their LM half, ...
        const int blk = tid >> 7, j0 = (tid & 127) + 128 * (blk >> 1);
        if (blk & 1) { for (int j = j0; j < nsel; j += kThreads / 2) place_lm(j, sel[j]); }
        else { for (int j = j0; j < nsel; j += kThreads / 2) place_core(j, sel[j]); }
      } else {
        for (int j = tid; j < nsel; j += kThreads) place(j, sel[j]);
      }
    };
    if (nreal > W) {                                                             // :405-415
      // ---- radix select of the W-th largest score on the order-preserving 64-bit key, 11 bits per pass ----
      // Where to start: the threshold lies between the smallest score of a full beam's old members (W candidates are
      // at least that good) and the largest score of all, so it shares their common leading bits (s_hi / s_lo).
      // Starting below them, the first digit already spreads the candidates that matter over the bins (a pass over
      // the sign/exponent bits would put all of them into one): 1.01 passes per step measured.  A pass stops the
      // search as soon as the bin of the chosen digit holds exactly the remaining k (taken whole) or at most 64
      // candidates (ranked exactly below).  Two histograms alternate; both start the step cleared.
      const unsigned H32 = s_hi, L32 = n == W ? s_lo : 0u;
      const unsigned xdiff = H32 ^ L32;
      const int hb = xdiff ? 63 - __builtin_clz(xdiff) : 31;                    // highest bit that may differ
      unsigned long long mask = hb == 63 ? 0ULL : ~0ULL << (hb + 1);
      unsigned long long prefix = ((unsigned long long)H32 << 32) & mask;       // (decided bits: the same in every thread)
      int krem = W, bin = 0;
      bool done = false;
      int shift = hb + 1 - kSelBits;                                            // >= 21
      for (int pass = 0;; pass++) {
        int* hcur = hist + (pass & 1) * kSelBins;
        int* hnext = hist + ((pass & 1) ^ 1) * kSelBins;
        const int nbits = 64 - __builtin_popcountll(mask) - shift;                    // (the last digit may be short)
        const int width = nbits < kSelBits ? nbits : kSelBits;
        const unsigned long long dmask = (1ULL << width) - 1ULL;
        for (int d = tid; d < ntot; d += kThreads) {
          const unsigned long long u = ukey[d];
          if ((u & mask) == prefix && u != kNoCandKey) atomicAdd(&hcur[(int)((u >> shift) & dmask)], 1);
        }
        lds_barrier();
        // (hnext: at pass 0 the region that held the previous step's sel)
        const unsigned long long digit_mask = dmask << shift;
        select_digit<LdsSync>(hcur, hnext, krem, s_part, [&](int rest, int digit, int count) {
          s_krem = rest;
          s_prefix = (prefix & ~digit_mask) | ((unsigned long long)digit << shift);
          s_bin = count;
          s_done = count == rest ? 1 : 0;     // the whole bin survives: no finer threshold needed
        });
        mask |= digit_mask;
        lds_barrier();
        krem = s_krem; prefix = s_prefix; bin = s_bin; done = s_done != 0;
#ifdef E2E_BEAM_PROFILE
        if (b == 0 && tid == 0) g_beam_prof[10] += 1;
#endif
        if (done || shift == 0 || bin <= kSelSmall) break;
        shift = shift - kSelBits > 0 ? shift - kSelBits : 0;
        lds_barrier();                                // (s_* are rewritten by the next pass)
      }
      BPROF(7);
      // Gathered for the final ranking: keys whose decided bits are above the threshold prefix, plus those equal to
      // it -- all of them if they are at most 64 (the ranking below keeps the best krem of them), else exactly krem:
      // the whole bin, or (every bit decided: exact ties) the first by position.
      const unsigned long long Tk = prefix;
      const bool small_bin = !done && shift != 0;           // (then bin <= kSelSmall and bin > krem)
#define OKEY_CMP(u) ((u) & mask)
      // ---- compaction: larger keys first, then the equal ones ----
      const int per = (ntot + kThreads - 1) / kThreads;
      const int d0 = min(tid * per, ntot), d1 = min(d0 + per, ntot);
      int ngt = 0, neq = 0;
      unsigned cls = 0;                              // two bits per candidate of this thread: 1 above, 2 in the threshold bin
      static_assert(kMaxCand <= 16 * kThreads, "classification bits per thread");
      for (int d = d0, sh2 = 0; d < d1; d++, sh2 += 2) {
        const unsigned long long uf = ukey[d], u = OKEY_CMP(uf);
        const bool gt = u > Tk, eq = u == Tk && uf != kNoCandKey;
        ngt += gt; neq += eq;
        cls |= (gt ? 1u : eq ? 2u : 0u) << sh2;
      }
      // (both counts ride in one integer -- at most 8192 candidates, 16 bits each -- through one wave scan, and the 16
      // waves' totals through one 16-lane scan instead of a 16-step loop in every wave)
      const int iboth = wave_scan_i(ngt | (neq << 16));
      if (lane == 63) s_part[wid] = iboth;
      lds_barrier();
      const int wtot = wave_scan_i(lane < kThreads / 64 ? s_part[lane] : 0);
      const int wbase = wid > 0 ? __builtin_amdgcn_readlane(wtot, wid - 1) : 0;
      const int tg = __builtin_amdgcn_readlane(wtot, kThreads / 64 - 1) & 0xffff;
      const int mine_excl = wbase + iboth - (ngt | (neq << 16));
      int og = mine_excl & 0xffff, oe = mine_excl >> 16;
      const int take = small_bin ? bin : krem;
      for (int d = d0; d < d1 && cls; d++, cls >>= 2) {
        if (cls & 1u) { uskey[og] = ukey[d]; sidx[og] = d; og++; }
        else if (cls & 2u) {
          if (oe < take) { uskey[tg + oe] = ukey[d]; sidx[tg + oe] = d; }
          oe++;
        }
      }
#undef OKEY_CMP
      const int M = tg + take;                      // W <= M <= W - 1 + kSelSmall gathered candidates
      lds_barrier();
      BPROF(8);
      // ---- rank the gathered candidates; rank < W is the candidate's place in the new beam (the surplus of a small
      //      threshold bin falls off the end) ----
      if (LM) for (int h = tid; h < kStateSlots; h += kThreads) tsig[h] = 0ULL;
      rank_gathered<4>(uskey, M, W, [&](int rank, int e) { sel[rank] = sidx[e]; });
      place_all();
    } else {
      // nothing is pruned (the first steps of an utterance): old members, then the pairs that exist, in order
      for (int j = tid; j < n; j += kThreads) sel[j] = j;
      const int chunk = (npairs + kThreads - 1) / kThreads;
      const int q0 = min(tid * chunk, npairs), q1 = min(q0 + chunk, npairs);
      int mine = 0;
      for (int q = q0; q < q1; q++) mine += ukey[n + q] != kNoCandKey;
      const int incl = wave_scan_i(mine);
      if (lane == 63) s_part[wid] = incl;
      lds_barrier();
      int pos = n + incl - mine;
      for (int w = 0; w < wid; w++) pos += s_part[w];
      for (int q = q0; q < q1; q++)
        if (ukey[n + q] != kNoCandKey) sel[pos++] = n + q;
      if (LM) for (int h = tid; h < kStateSlots; h += kThreads) tsig[h] = 0ULL;
      place_all();
    }
    lds_barrier();
    BPROF(3);
    rebuild_guards(A, Bm, nsel, V, [&](int e, int node) { ctabB[e] = node; });
    if (LM) {
      // The LM's answers for the new beam: carried over with a member that stays, asked for a member that is new -- but
      // only once per LM STATE.  What is asked depends on the member's state only (the word begun, the context, whether
      // a word starts), and most new members share theirs with another member: prefixes that differ further back than
      // the model looks (measured: 70 new members per step, 22 distinct states).  A wave walks the whole query code as
      // soon as one of its lanes has a query, so the queries are packed: one (asking member, character) per thread.
      //   1. every member looks its state's signature up in a small hash table: a member that stays enters itself (its
      //      answers are already there), a new member follows the holder if there is one and it really has the same state
      //      (the signature is a filter), else it enters itself, asks, and joins the packed list;
      //   2. rows are copied (staying members) / asked (list);  3. followers copy their leader's row.
      BPROF(11);
      auto state_of = [&](int j2, bool& nw, int& cn, unsigned long long& wh) {
        const LmFields& m = Bm.lm[j2];
        nw = m.num_words == 0 || Bm.last[j2] == p.space_id;
        cn = nw ? m.st_n : m.stb_n;
        wh = nw ? 0ULL : m.word_hash;
      };
      // One pass, on the threads next to the ones that walk the guards above (tid ^ 128: the two loops are independent).  A
      // table word is the state's signature with the holder's position in its low 12 bits.  A member that stays makes
      // itself the holder (smallest position wins); a new member takes a free word -- it is then the one that asks -- or
      // finds a holder and, if that really has the same state, follows it.  Whoever holds a state when a new member comes
      // by will have its row in time (copied below, or asked in the next phase); which of several equal-state members
      // that is changes nothing but who asks.
      for (int j2 = tid ^ 128; j2 < nsel; j2 += kThreads) {
        bool nw; int cn; unsigned long long wh;
        state_of(j2, nw, cn, wh);
        unsigned long long h = wh;
        for (int q2 = 0; q2 < cn; q2++) h = ng_mix(h, nw ? Bm.lm[j2].st[q2] : Bm.lm[j2].stb[q2]);
        h = ng_mix(h, (uint32_t)cn + (nw ? 100u : 0u));
        unsigned long long hk = h & ~0xFFFULL;
        if (hk == 0) hk = 0x1000ULL;
        const bool stays = Bm.from[j2] >= 0;
        int leader = j2;
        for (unsigned sl = (unsigned)(h >> 20) & (kStateSlots - 1);; sl = (sl + 1) & (kStateSlots - 1)) {
          const unsigned long long old = atomicCAS(&tsig[sl], 0ULL, hk | (unsigned long long)j2);
          if (old == 0ULL) break;                              // the word is this member's
          if ((old & ~0xFFFULL) != hk) continue;
          if (stays) { atomicMin(&tsig[sl], hk | (unsigned long long)j2); break; }
          const int o = (int)(old & 0xFFFULL);
          bool nw2; int cn2; unsigned long long wh2;
          state_of(o, nw2, cn2, wh2);
          bool same = nw2 == nw && cn2 == cn && wh2 == wh;
          for (int q2 = 0; q2 < cn && same; q2++)
            same = (nw ? Bm.lm[o].st[q2] : Bm.lm[o].stb[q2]) == (nw ? Bm.lm[j2].st[q2] : Bm.lm[j2].stb[q2]);
          if (same) { leader = o; break; }                    // (else: another state behind the same signature bits -- next word)
        }
        if (!stays && leader == j2) {
          newlist[atomicAdd(&s_nnew, 1)] = j2;
#ifdef E2E_BEAM_PROFILE
          if (b == 0) { const int q9 = atomicAdd(&g_beam_nsig, 1); if (q9 < (1 << 17)) g_beam_sigs[q9] = h; }
#endif
        }
        ldr[j2] = leader;
      }
      // (the rows of the members that stay: the waves behind those two copy them meanwhile)
      for (int e = tid - 256; e >= 0 && e < nsel * V; e += kThreads - 256) {
        const int j2 = div_v(e);
        const int f = Bm.from[j2];
        if (f >= 0) lmcB[e] = lmcA[f * V + (e - j2 * V)];
      }
      lds_barrier();
      BPROF(13);
      const int nnew = s_nnew;
      for (int t2 = tid; t2 < nnew * V; t2 += kThreads) {
        const int r = div_v(t2), c = t2 - r * V, j2 = newlist[r];
        if (c == blank || c == p.space_id) continue;
        lmcB[j2 * V + c] = lm_query<lmk_fast(LMK), RS, lmk_hom(LMK)>(p, lt, Bm.lm[j2], Bm.last[j2], c);
      }
      lds_barrier();
      BPROF(14);
      for (int e = tid; e < nsel * V; e += kThreads) {
        const int j2 = div_v(e);
        const int o = ldr[j2];
        if (o != j2) lmcB[e] = lmcB[o * V + (e - j2 * V)];
      }
    }
    if (tid < V) srow2[((t + 1) & 1) * V + tid] = next_lp;          // (the other half of the double buffer: nobody reads it this step)
    lds_barrier();
    BPROF(5);
    n = nsel; cur ^= 1;
    if (s_err) break;
  }

  Members A;
  A.carve(mem0 + (size_t)cur * mbytes, W);
  // (the n-best read-out's scratch: the candidate keys and the selection's two histograms, dead after the last step)
  if (ST) stream_suspend(p, st_row, mem0 + (size_t)cur * mbytes, mbytes, n, s_next_node, t0, T, s_err);
  if (p.nbest) read_out_nbest<LM>(p, A, n, reinterpret_cast<unsigned long long*>(key), hist, hist + kSelBins, nodes, node_t, s_err);
  else if (!ST) read_out<LM>(p, A, n, key, nodes, s_err);               // (a stream fed with nbest = 0 reads nothing out)
}

// entry k of the table is instance k: the pack expands LMK = 0 .. kLmKinds - 1 in order
template <typename IO, bool ST, int... LMK>
const void* lds_instance(int lmk, std::integer_sequence<int, LMK...>) {
  static const void* const instances[] = { reinterpret_cast<const void*>(&ctc_beam_kernel<IO, LMK, ST>)... };
  return instances[lmk];
}

}  // namespace

template <> const void* lds_kernel<E2E_BEAM_IO>(int lmk, bool st) {
  using Kinds = std::make_integer_sequence<int, kLmKinds>;
  return st ? lds_instance<E2E_BEAM_IO, true>(lmk, Kinds()) : lds_instance<E2E_BEAM_IO, false>(lmk, Kinds());
}

}  // namespace beamk
}  // namespace e2e

#ifdef E2E_BEAM_PROFILE
extern "C" int e2e_debug_beam_sigs(unsigned long long* host, int cap) {
  int n = 0;
  if (hipMemcpyFromSymbol(&n, HIP_SYMBOL(g_beam_nsig), sizeof(int)) != hipSuccess) return -1;
  if (n > cap) n = cap;
  if (n > (1 << 17)) n = 1 << 17;
  if (hipMemcpyFromSymbol(host, HIP_SYMBOL(g_beam_sigs), sizeof(unsigned long long) * n) != hipSuccess) return -1;
  const int zero = 0;
  (void)hipMemcpyToSymbol(HIP_SYMBOL(g_beam_nsig), &zero, sizeof(int));
  return n;
}
extern "C" int e2e_debug_beam_profile(unsigned long long* host) {
  if (hipDeviceSynchronize() != hipSuccess) return E2E_ERR_HIP;
  return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_beam_prof), sizeof(unsigned long long) * 16) == hipSuccess ? 0 : E2E_ERR_HIP;
}
#endif
