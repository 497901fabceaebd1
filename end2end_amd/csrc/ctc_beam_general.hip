// ------------------------------------------------------------------------------------------------------
// The general form: any alphabet width
// ------------------------------------------------------------------------------------------------------
// ctc_beam_kernel (ctc_beam_lds.hip) keeps everything that scales with beam_width * alphabet in LDS -- candidate keys, the
// members' child tables, the LM's answers -- which bounds the width by the alphabet (81 at V = 80, 7 at V = 1000).  This one is the same
// algorithm, phase by phase, with those three in HBM (L2-resident: 16-24 bytes per (member, character)):
//   * candidate keys: an array in the workspace, streamed by the pair loop (written) and by the radix select and the
//     gather (read); the select starts below the leading bits that the best score and the worst old member share, as
//     there, and runs on to the last bit (no small-bin finish);
//   * child tables: at most one alive child per member is ever recorded (its guard), so a step's table is a hash map
//     of <= W entries keyed by (member position, character) in LDS instead of W*V words;
//   * the LM's answers: rows in the workspace, copied with a member that stays, asked for a member that is new (every
//     new member asks for itself: no sharing between members of equal LM state);
//   * the frame's log-probabilities are read from the input where they are needed (no staging).
// Barriers are full (__syncthreads after a workgroup fence): data crosses threads through global memory here.
// Not tuned: it exists so that an alphabet the fast kernel cannot hold is decoded at all, on the device, with
// the same result (tests run the whole beam suite through it: E2E_BEAM_GENERAL=1).  beam_width <= kGenMaxW and what the
// maps and the selection's arrays leave of one workgroup's LDS (the member sets move to the workspace beyond ~256): 512.
//
// Compiled once per input dtype like ctc_beam_lds.hip, and once more for the pruned calls (-DE2E_BEAM_CUT=false / true):
// ctc_beam_general.f32.o, ... with general_kernel<IO, false>, ctc_beam_general_cut.f32.o, ... with general_kernel<IO, true>.  GenParams, kGenMaxW
// and the sizes of the character pre-selection are in ctc_beam_common.h: the host lays the workspace out with them.
#include <utility>

#include "ctc_beam_common.h"

namespace e2e {
namespace beamk {
namespace {      // (the kernels have internal linkage: only the table below names them)

// order-preserving 32-bit key of a float (larger value -> larger key; -0 < +0 does not matter here)
__device__ __forceinline__ unsigned okey32(float f) {
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ void gsync() { __threadfence_block(); __syncthreads(); }

// is label c in the frame's ascending list l[0 .. n)?  (a pruned call: the member's own last label)
__device__ __forceinline__ bool cut_has(const int* l, int n, int c) {
  int lo = 0, hi = n;
  while (lo < hi) { const int m = (lo + hi) >> 1; if (l[m] < c) lo = m + 1; else hi = m; }
  return lo < n && l[lo] == c;
}

template <typename IO, int LMK, bool ST, bool CUT>
__global__ __launch_bounds__(kThreads) void ctc_beam_general_kernel(BeamParams p, GenParams g) {
  constexpr bool LM = LMK != 0, RS = lmk_restricted(LMK);
  extern __shared__ __align__(16) unsigned char smem[];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int V = p.V, W = p.W, blank = p.blank;
  // ---- LDS carve-up ----
  unsigned char* q8 = smem;
  // the two member sets: LDS while they fit beside the rest, else the workspace (beams of several hundred hypotheses:
  // every access to a member then goes to L2 -- slower per step, but upstream has no bound on the width at all)
  const size_t mbytes = Members::bytes(W);
  unsigned char* const mem0 = g.gmem ? g.gmem + (size_t)blockIdx.x * 2 * mbytes : q8;
  if (!g.gmem) q8 += 2 * mbytes;
  unsigned long long* uskey = (unsigned long long*)q8; q8 += sizeof(unsigned long long) * (p.WP2 + 8);
  double* fkey = (double*)q8; q8 += sizeof(double) * (p.WP2 + 8);          // final scores
  int* sidx = (int*)q8; q8 += sizeof(int) * (p.WP2 + 8);
  int* hist = (int*)q8; q8 += sizeof(int) * kSelBins;
  int* s_part = (int*)q8; q8 += sizeof(int) * 64;
  int* const sm0 = (int*)q8; q8 += sizeof(int) * 4 * p.HS;                  // [set][key | val][HS]  node -> position
  int* const cm0 = (int*)q8; q8 += sizeof(int) * 4 * g.CH;                  // [set][key | val][CH]  (position, char) -> child node
  int* const s_lst = (int*)q8; q8 += sizeof(int) * gen_list_cap(W);         // this step's characters, ascending
  unsigned* const s_bits = (unsigned*)q8; q8 += sizeof(unsigned) * gen_bitmap_words(V);   // one bit per character
  auto slot_map = [&](int set) { SlotMap m; m.key = sm0 + set * 2 * p.HS; m.val = m.key + p.HS; m.mask = p.HS - 1; return m; };
  auto child_map = [&](int set) { ChildMap m; m.key = cm0 + set * 2 * g.CH; m.val = m.key + g.CH; m.mask = g.CH - 1; return m; };
  __shared__ int s_next_node, s_err, s_krem, s_done, s_total_new, s_nl;
  __shared__ unsigned s_fmax, s_ckey;
  __shared__ unsigned s_hi, s_lo;
  __shared__ unsigned long long s_prefix;
  LabelTab lt; lt.off = p.lm.label_off; lt.bytes = p.lm.label_bytes; lt.one = nullptr;

  unsigned char* const st_row = ST ? p.st_rows + (size_t)b * p.st_row_bytes : nullptr;     // (streaming: see the fast kernel)
  BeamNode* nodes = ST ? reinterpret_cast<BeamNode*>(st_row + p.st_nodes_off) : p.nodes + (size_t)b * p.NCAP;
  int* const node_t = ST ? (p.st_ts_off ? reinterpret_cast<int*>(st_row + p.st_ts_off) : nullptr)
                         : p.node_t ? p.node_t + (size_t)b * p.NCAP : nullptr;         // (uniform: null in the plain call)
  const IO* lp = reinterpret_cast<const IO*>(p.lp) + (int64_t)b * p.sB;
  // A pruned call (e2e_ctc_beam_nbest_cut: the CUT instances, objects of their own): a step expands the frame's label list and
  // nothing of it scales with V -- no answer rows: the pair loop asks the LM for the pairs that have no living child, `place`
  // asks again for the <= W children it creates (W queries a frame against a stash of W * (K+1) answers written for W read).
  // (A run-time branch on g.cut_ids instead of the template argument cost the unpruned call 4 % at V = 8000, W = 100: DESIGN.md 4.4.)
  constexpr bool cut = CUT;
  unsigned long long* const gkey = g.gkey + (size_t)b * (CUT ? g.gstride : (size_t)W + (size_t)W * V);
  LmAnswer* const lmc0 = LM && !cut ? g.lmc + (size_t)b * 2 * (size_t)W * V : nullptr;
  int64_t Tq = p.x_len[b];
  const int T = Tq < 0 ? 0 : (Tq > p.T ? p.T : (int)Tq);
  Members M0; M0.carve(mem0, W);
  int t0 = 0, n0 = 1;
  bool resume = false;
  if (ST) {
    t0 = stream_open(p, st_row, T, resume);
    if (t0 < 0) { stream_refuse(p, t0); return; }
    if (resume) n0 = __builtin_amdgcn_readfirstlane(reinterpret_cast<const StreamHeader*>(st_row)->n);
  }

  for (int h = tid; h < 2 * p.HS; h += kThreads) { sm0[h] = -1; sm0[2 * p.HS + h] = -1; }
  for (int h = tid; h < 2 * g.CH; h += kThreads) { cm0[h] = -1; cm0[2 * g.CH + h] = -1; }
  if (tid == 0) {
    s_next_node = 1; s_err = 0;                                                     // node 0 is taken
    if (!ST || !resume) init_root(p, nodes, M0);
    else s_next_node = reinterpret_cast<const StreamHeader*>(st_row)->next_node;
  }
  if (ST && resume) stream_load_members(mem0, st_row, mbytes);
  gsync();
  if (!ST || !resume) {
    if (tid == 0) slot_map(0).insert(0, 0);
    if (LM && !cut) for (int c = tid; c < V; c += kThreads) if (c != blank && c != p.space_id) lmc0[c] = lm_query<lmk_fast(LMK), RS, lmk_hom(LMK)>(p, lt, M0.lm[0], -1, c);
  } else {
    // what a step rebuilds: the slot map, the child map (one entry per guard) and the members' LM answer rows
    const SlotMap map0 = slot_map(0);
    const ChildMap cm = child_map(0);
    for (int i = tid; i < n0; i += kThreads) {
      map0.insert(M0.node[i], i);
      const int go = M0.gown[i];
      if (go >= 0) cm.insert(go * V + M0.gchar[i], M0.gnode[i]);
    }
    if (LM && !cut) for (size_t e = tid; e < (size_t)n0 * V; e += kThreads) {
      const int j2 = (int)(e / V), c = (int)(e - (size_t)j2 * V);
      if (c != blank && c != p.space_id) lmc0[e] = lm_query<lmk_fast(LMK), RS, lmk_hom(LMK)>(p, lt, M0.lm[j2], M0.last[j2], c);
    }
  }
  gsync();
  int n = n0, cur = 0;
  // q / n for the candidate numbers of a step (q < n * V, q * n < 2^32) by one multiplication: ceil(2^32 / n), worked out when
  // the beam's size changes (a division per candidate was a third of the pair loop's instructions at ~30 candidates per thread)
  // (exact while q * n < 2^32; a beam of 512 over an alphabet of 32 000 without the pre-selection is beyond that: plain division)
  int magic_n = -1; unsigned magic = 0u; bool magic_ok = false;
  auto div_n = [&](int q) -> int { return magic_ok ? (int)__umulhi((unsigned)q, magic) : q / n; };

  for (int t = 0; t < T; t++) {
    if (n != magic_n) {
      magic_n = n; magic = n > 1 ? (unsigned)((0x100000000ULL + (unsigned)n - 1u) / (unsigned)n) : 0u;
      magic_ok = n > 1 && (unsigned long long)n * (unsigned long long)V * (unsigned long long)n < (1ULL << 32);
    }
    Members A, Bm;
    A.carve(mem0 + (size_t)cur * mbytes, W);
    Bm.carve(mem0 + (size_t)(cur ^ 1) * mbytes, W);
    const SlotMap mapA = slot_map(cur), mapB = slot_map(cur ^ 1);
    const ChildMap cmA = child_map(cur), cmB = child_map(cur ^ 1);
    const LmAnswer* const lmcA = LM && !cut ? lmc0 + (size_t)cur * W * V : nullptr;
    LmAnswer* const lmcB = LM && !cut ? lmc0 + (size_t)(cur ^ 1) * W * V : nullptr;
    const int* const cl = cut ? g.cut_ids + ((size_t)b * p.T + t) * g.cut_k1 : nullptr;     // this frame's labels, ascending
    const IO* const row = lp + (int64_t)t * p.sT;
    auto LP = [&](int c) -> double { return (double)row[(int64_t)c * p.sV]; };
    if (tid == 0) { s_hi = 0u; s_lo = 0xffffffffu; s_total_new = 0; }
    for (int h = tid; h < kSelBins; h += kThreads) hist[h] = 0;
    __syncthreads();
    // ---- which characters can matter this step (no language model) ----
    // Without a language model the score of a would-be prefix (i, c) is lp[c] + full_i - wip * words, monotone in lp[c] for a
    // given prefix except for c = the prefix's last character (it extends from ppb_i) and c = space (the word count).  A
    // prefix has at most m_i <= W characters whose child already lives (no candidate), so its candidate of rank > 2W in
    // lp order has >= W candidates of the same prefix before it in the reference's order (score desc, position asc: equal
    // lp, lower c first) and cannot be among the W survivors.  The step therefore scores, for every prefix, only
    // L = {the 2W largest lp[c], every c tied with the last of them} + {space} + {last_i}, in ascending c so that the order
    // of the keys stays the reference's: |L| * n <= (3W + 1) * W keys instead of V * n (10 k instead of 800 k at V = 8000,
    // W = 100).  Exact unless two DIFFERENT lp values could round to the same score, i.e. unless |full| is within 2^24 of
    // their spacing: f32 inputs and |full| < 2^20 only; otherwise, with a language model, for tiny alphabets or if the ties
    // overflow the list, every character is taken as before.
    bool pre = !cut && LMK == 0 && sizeof(IO) <= 4 && V <= 65536 && V - 1 > 3 * W + 2;      // (16-bit inputs are f32 numbers too)
    if (pre) {
      if (tid == 0) s_fmax = 0u;
      __syncthreads();
      unsigned fm = 0u;
      for (int i = tid; i < n; i += kThreads) fm = max(fm, __float_as_uint(fabsf((float)A.full[i])));
      fm = (unsigned)wave_max_i((int)fm);
      if (lane == 0 && fm) atomicMax(&s_fmax, fm);
      __syncthreads();
      pre = __uint_as_float(s_fmax) < 1048576.f;
    }
    int NL = cut ? min(g.cut_n[(size_t)b * p.T + t], g.cut_k1) : V;
    if (pre) {
      // threshold: the key of the (2W)-th largest lp[c], c != blank -- radix select over V 32-bit keys, 11 bits per pass
      const int want = 2 * W;
      unsigned prefix = 0u, maskc = 0u;
      int krem = want;
      for (int pass = 0; pass < 3; pass++) {
        const int shift = pass == 0 ? 21 : pass == 1 ? 10 : 0, width = pass == 2 ? 10 : 11;
        for (int c = tid; c < V; c += kThreads) {
          if (c == blank) continue;
          const unsigned u = okey32((float)LP(c));
          if ((u & maskc) == prefix) atomicAdd(&hist[(int)((u >> shift) & ((1u << width) - 1u))], 1);
        }
        __syncthreads();
        select_digit<FullSync>(hist, hist, krem, s_part, [&](int rest, int digit, int) { s_krem = rest; s_ckey = prefix | ((unsigned)digit << shift); });
        __syncthreads();
        krem = s_krem; prefix = s_ckey; maskc |= ((1u << width) - 1u) << shift;
        __syncthreads();
      }
      const unsigned Tk = prefix;                        // every c with key >= Tk is taken (ties with the 2W-th included)
      const int words = (V + 31) / 32;
      for (int wd = tid; wd < words; wd += kThreads) s_bits[wd] = 0u;
      __syncthreads();
      for (int c = tid; c < V; c += kThreads)
        if (c != blank && okey32((float)LP(c)) >= Tk) atomicOr(&s_bits[c >> 5], 1u << (c & 31));
      if (tid == 0 && p.space_id >= 0 && p.space_id < V && p.space_id != blank) atomicOr(&s_bits[p.space_id >> 5], 1u << (p.space_id & 31));
      for (int i = tid; i < n; i += kThreads) { const int lc = A.last[i]; if (lc >= 0 && lc != blank) atomicOr(&s_bits[lc >> 5], 1u << (lc & 31)); }
      __syncthreads();
      // the list, ascending: word wd's characters start at the number of bits set before it
      int run = 0;                                       // (bits set in the words of earlier rounds)
      for (int w0 = 0; w0 < words; w0 += kThreads) {
        const int wd = w0 + tid;
        const unsigned bits = wd < words ? s_bits[wd] : 0u;
        const int pc = __builtin_popcount(bits);
        const int inc = wave_scan_i(pc);
        if (lane == 63) s_part[wid] = inc;
        __syncthreads();
        int off = run + inc - pc, tot = 0;
        for (int w2 = 0; w2 < kThreads / 64; w2++) { if (w2 < wid) off += s_part[w2]; tot += s_part[w2]; }
        unsigned bb = bits;
        while (bb) { const int bit = __builtin_ctz(bb); bb &= bb - 1; if (off < gen_list_cap(W)) s_lst[off] = wd * 32 + bit; off++; }
        run += tot;
        __syncthreads();
      }
      if (tid == 0) s_nl = run;
      __syncthreads();
      NL = s_nl;
      if (NL > gen_list_cap(W)) { pre = false; NL = V; }        // (more ties than the list holds: every character)
    }
    auto CH = [&](int sidx) -> int { return cut ? cl[sidx] : pre ? s_lst[sidx] : sidx; };
    // (pruned: a member's last label outside the frame's list gives the member no repeated-label share)
    auto LPm = [&](int c) -> double { return !cut || cut_has(cl, NL, c) ? LP(c) : ninf(); };
    // (pruned: the LM's answer for the child (member i, label c), asked when it is needed; the space asks nothing)
    auto cut_answer = [&](int i, int last, int c) -> LmAnswer {
      LmAnswer a; a.sc = 0.f; a.wi = 0u;
      if (c != p.space_id) a = lm_query<lmk_fast(LMK), RS, lmk_hom(LMK)>(p, lt, A.lm[i], last, c);
      return a;
    };
    // ---- pairs: candidate q = c*n + i is the reference's order (character outer, prefix inner, :370-395) ----
    // (the blank creates no candidate: its share of every member is taken first)
    for (int i = tid; i < n; i += kThreads) A.npb[i] = LP(blank) + A.full[i];      // :374-376 (prob_blank was -inf)
    const int npairs = n * NL;
    int my_new = 0;
    unsigned key_hi = 0u, key_lo = 0xffffffffu;
    for (int e = tid; e < npairs; e += kThreads) {
      const int si = div_n(e), ii = e - si * n;        // (slot si of the list outer, prefix inner: the reference's order)
      const int ci = CH(si);
      const double full = A.full[ii], ppb = A.ppb[ii];
      const int last = A.last[ii];
      const double curp = LP(ci);
      unsigned long long* const slot = gkey + n + e;
      if (ci == blank || (cut && (unsigned)ci >= (unsigned)V)) { *slot = kNoCandKey; continue; }
      const double val = curp + (ci == last ? ppb : full);                     // :383-385 / :389-391
      const int k = cmA.find(ii * V + ci);
      unsigned long long uk = kNoCandKey;
      if (k >= 0) {
        const int j = mapA.find(k);
        if (j >= 0) A.inc[j] = val;            // the child is a beam member: its share from this parent
        // else: alive but pruned (Q7) -- the probability is lost and the slot stays taken
      } else {
        const LmFields pr = score_fields<LM>(A.lm[ii]);
        const LmAnswer ans = LM && cut ? cut_answer(ii, last, ci) : answer_at<LM>(lmcA, (size_t)ii * V + ci);
        if (!RS || !lexicon_forbids(p, pr, last, ci, ans)) {
          uk = child_key<LM>(p, pr, last, ci, ans, val);
          key_hi = max(key_hi, (unsigned)(uk >> 32));
          my_new++;
        }
      }
      *slot = uk;
    }
    {
      const int incl = wave_scan_i(my_new);
      if (lane == 63 && incl) atomicAdd(&s_total_new, incl);
    }
    gsync();
    update_members<LM>(p, A, n, LPm, gkey, key_hi, key_lo);
    key_hi = (unsigned)wave_max_i((int)(key_hi ^ 0x80000000u)) ^ 0x80000000u;
    key_lo = ~((unsigned)wave_max_i((int)((~key_lo) ^ 0x80000000u)) ^ 0x80000000u);
    if (lane == 0) { atomicMax(&s_hi, key_hi); atomicMin(&s_lo, key_lo); }
    for (int h = tid; h < p.HS; h += kThreads) mapB.key[h] = -1;
    for (int h = tid; h < g.CH; h += kThreads) cmB.key[h] = -1;
    gsync();
    const int total_new = s_total_new;
    const int nreal = n + total_new;                // candidates that exist
    const size_t ntot = (size_t)n + (size_t)npairs; // entries of gkey[]
    const int nsel = nreal > W ? W : nreal;
    // candidate d takes place j of the new beam (see the fast kernel's `place`)
    auto place = [&](int j, int d) {
      if (d < n) {
        const int i = d;
        A.kept[i] = 1; A.newpos[i] = j; Bm.from[j] = i;
        Bm.ppb[j] = A.npb[i]; Bm.ppnb[j] = A.npnb[i]; Bm.full[j] = A.nfull[i];
        Bm.node[j] = A.node[i]; Bm.last[j] = A.last[i]; copy_lm<LM>(Bm.lm[j], A.lm[i]);
        Bm.gown[j] = A.gown[i]; Bm.gchar[j] = A.gchar[i]; Bm.gnode[j] = A.gnode[i];
        mapB.insert(A.node[i], j);
      } else {
        const int q = d - n;
        const int si = div_n(q), i = q - si * n;
        const int c = CH(si);
        const double val = LP(c) + (c == A.last[i] ? A.ppb[i] : A.full[i]);
        child_lm<LM>(p, lt, A.lm[i], A.last[i], c,
                     LM && cut ? cut_answer(i, A.last[i], c) : answer_at<LM>(lmcA, (size_t)i * V + c), Bm.lm[j]);
        int k = atomicAdd(&s_next_node, 1);                                       // make_shared<Prefix>, :254
        if (k >= p.NCAP) { s_err = 1; k = 0; }
        else {
          BeamNode nn;
          nn.parent = A.node[i]; nn.last_char = c;
          nodes[k] = nn;
          if (node_t) node_t[k] = ST ? t0 + t : t;
          mapB.insert(k, j);
        }
        Bm.ppb[j] = ninf(); Bm.ppnb[j] = val; Bm.full[j] = lse2(val, ninf()); Bm.node[j] = k; Bm.last[j] = c;
        Bm.gown[j] = i; Bm.gchar[j] = c; Bm.gnode[j] = k;
        Bm.from[j] = -1;
      }
    };
    // this thread's contiguous chunk of candidate positions (ordered passes below)
    const size_t per = (ntot + kThreads - 1) / kThreads;
    const size_t d0 = min((size_t)tid * per, ntot), d1 = min(d0 + per, ntot);
    if (nreal > W) {                                                             // :405-415
      // ---- radix select of the W-th largest key, 11 bits per pass, from the first bit that can differ ----
      const unsigned H32 = s_hi, L32 = n == W ? s_lo : 0u;
      const unsigned xdiff = H32 ^ L32;
      const int hb = xdiff ? 63 - __builtin_clz(xdiff) : 31;
      unsigned long long mask = hb == 63 ? 0ULL : ~0ULL << (hb + 1);
      unsigned long long prefix = ((unsigned long long)H32 << 32) & mask;
      int krem = W;
      bool done = false;
      int shift = hb + 1 - kSelBits;
      for (;;) {
        const int nbits = 64 - __builtin_popcountll(mask) - shift;
        const int width = nbits < kSelBits ? nbits : kSelBits;
        const unsigned long long dmask = (1ULL << width) - 1ULL;
        for (size_t d = tid; d < ntot; d += kThreads) {
          const unsigned long long u = gkey[d];
          if ((u & mask) == prefix && u != kNoCandKey) atomicAdd(&hist[(int)((u >> shift) & dmask)], 1);
        }
        __syncthreads();
        const unsigned long long digit_mask = dmask << shift;
        select_digit<FullSync>(hist, hist, krem, s_part, [&](int rest, int digit, int count) {
          s_krem = rest;
          s_prefix = (prefix & ~digit_mask) | ((unsigned long long)digit << shift);
          s_done = count == rest ? 1 : 0;     // the whole bin survives: no finer threshold needed
        });
        mask |= digit_mask;
        __syncthreads();
        krem = s_krem; prefix = s_prefix; done = s_done != 0;
        if (done || shift == 0) break;
        shift = shift - kSelBits > 0 ? shift - kSelBits : 0;
        __syncthreads();
      }
      // ---- gather: keys above the threshold, then the first krem of those equal to it, in position order ----
      const unsigned long long Tk = prefix;
      int ngt = 0, neq = 0;
      for (size_t d = d0; d < d1; d++) {
        const unsigned long long uf = gkey[d], u = uf & mask;
        ngt += u > Tk; neq += (u == Tk && uf != kNoCandKey);
      }
      const int igt = wave_scan_i(ngt), ieq = wave_scan_i(neq);
      if (lane == 63) { s_part[wid] = igt; s_part[16 + wid] = ieq; }
      __syncthreads();
      int og = igt - ngt, oe = ieq - neq, tg = 0;
      for (int w2 = 0; w2 < kThreads / 64; w2++) { if (w2 < wid) { og += s_part[w2]; oe += s_part[16 + w2]; } tg += s_part[w2]; }
      for (size_t d = d0; d < d1; d++) {
        const unsigned long long uf = gkey[d], u = uf & mask;
        if (u > Tk) { uskey[og] = uf; sidx[og] = (int)d; og++; }
        else if (u == Tk && uf != kNoCandKey) { if (oe < krem) { uskey[tg + oe] = uf; sidx[tg + oe] = (int)d; } oe++; }
      }
      const int M = tg + krem;                      // == W
      __syncthreads();
      rank_gathered<1>(uskey, M, W, [&](int rank, int e) { place(rank, sidx[e]); });
    } else {
      // nothing is pruned: old members, then the pairs that exist, in order
      int mine = 0;
      for (size_t d = max(d0, (size_t)n); d < d1; d++) mine += gkey[d] != kNoCandKey;
      const int incl = wave_scan_i(mine);
      if (lane == 63) s_part[wid] = incl;
      __syncthreads();
      int pos = n + incl - mine;
      for (int w2 = 0; w2 < wid; w2++) pos += s_part[w2];
      for (size_t d = max(d0, (size_t)n); d < d1; d++)
        if (gkey[d] != kNoCandKey) sidx[pos++] = (int)d;
      for (int j = tid; j < n; j += kThreads) sidx[j] = j;
      __syncthreads();
      for (int j = tid; j < nsel; j += kThreads) place(j, sidx[j]);
    }
    gsync();
    rebuild_guards(A, Bm, nsel, V, [&](int e, int node) { cmB.insert(e, node); });
    if (LM && !cut) {
      // the LM's answers for the new beam: rows copied with members that stay, asked for members that are new
      for (size_t e = tid; e < (size_t)nsel * V; e += kThreads) {
        const int j2 = (int)(e / V), c = (int)(e - (size_t)j2 * V);
        const int f = Bm.from[j2];
        if (f >= 0) lmcB[e] = lmcA[(size_t)f * V + c];
        else if (c != blank && c != p.space_id) lmcB[e] = lm_query<lmk_fast(LMK), RS, lmk_hom(LMK)>(p, lt, Bm.lm[j2], Bm.last[j2], c);
      }
    }
    gsync();
    n = nsel; cur ^= 1;
    if (s_err) break;
  }

  Members A;
  A.carve(mem0 + (size_t)cur * mbytes, W);
  if (ST) stream_suspend(p, st_row, mem0 + (size_t)cur * mbytes, mbytes, n, s_next_node, t0, T, s_err);
  if (p.nbest) read_out_nbest<LM>(p, A, n, reinterpret_cast<unsigned long long*>(fkey), sidx, hist, nodes, node_t, s_err);
  else if (!ST) read_out<LM>(p, A, n, fkey, nodes, s_err);
}

// entry k of the table is instance k: the pack expands LMK = 0 .. kLmKinds - 1 in order
template <typename IO, bool ST, bool CUT, int... LMK>
const void* general_instance(int lmk, std::integer_sequence<int, LMK...>) {
  static const void* const instances[] = { reinterpret_cast<const void*>(&ctc_beam_general_kernel<IO, LMK, ST, CUT>)... };
  return instances[lmk];
}

}  // namespace

template <> const void* general_kernel<E2E_BEAM_IO, E2E_BEAM_CUT>(int lmk, bool st) {
  using Kinds = std::make_integer_sequence<int, kLmKinds>;
  return st ? general_instance<E2E_BEAM_IO, true, E2E_BEAM_CUT>(lmk, Kinds()) : general_instance<E2E_BEAM_IO, false, E2E_BEAM_CUT>(lmk, Kinds());
}

}  // namespace beamk
}  // namespace e2e
