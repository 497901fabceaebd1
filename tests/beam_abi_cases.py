"""What tests/test_beam_abi_cpu.py holds the host side of the three beam searches to, and what tests/golden/make_beam_abi_golden.py
recorded of it from the commit before that host side was rewritten: the grid of workspace / row / width queries, and a list of
calls the C boundary refuses -- one argument error each, and two at once (the first error wins, so which of the two a call
reports says in what order the entry makes its checks).  Everything goes through _lib (ctypes); pointers are the dummy 256 that
is never dereferenced, because every call here is refused before any launch, with or without a GPU.
"""
import ctypes as C
import itertools

P = 256                                                                  # a pointer that is never dereferenced

# ---- the queries ----------------------------------------------------------------------------------------------------------------
CTC_B, CTC_T, CTC_V = (0, 1, 3, 64), (1, 40, 1500), (1, 5, 29, 300, 8000)
CTC_W = (1, 2, 16, 100, 256, 512, 513)


def ctc_top_ns(V):
    return (1, 4, 40, V, V + 1)


def query_grid():
    """{query name: [argument tuples]}: every branch of the layouts, and the arguments that must give 0."""
    g = {}

    def add(name, *args):
        g.setdefault(name, []).append(tuple(int(a) for a in args))
    pts = list(itertools.product(CTC_B, CTC_T, CTC_V, CTC_W, (0, 1), (0, 1)))
    pts += [(-1, 40, 29, 16, 1, 1), (3, 0, 29, 16, 1, 1), (3, 40, 0, 16, 1, 1), (3, 40, 29, 0, 1, 1), (3, 40, 29, -1, 0, 0)]
    for B, T, V, W, lm, ts in pts:
        add("e2e_ctc_beam_workspace_bytes", B, T, V, W)
        add("e2e_ctc_beam_workspace_bytes_lm", B, T, V, W, lm)
        add("e2e_ctc_beam_nbest_workspace_bytes", B, T, V, W, lm, ts)
        add("e2e_ctc_beam_stream_workspace_bytes", B, V, W, lm)
        add("e2e_ctc_beam_stream_row_bytes", T, V, W, lm, ts)             # (T: the stream's max_frames)
        for top_n in ctc_top_ns(V) + (0,):
            add("e2e_ctc_beam_cut_workspace_bytes", B, T, V, W, lm, ts, top_n)
            add("e2e_ctc_beam_cut_stream_workspace_bytes", B, T, V, W, lm, top_n)
        add("e2e_ctc_beam_max_width", V, lm)
        add("e2e_ctc_beam_cut_max_width", V, lm)
    for B, T, V, K, W in itertools.product((-1, 0, 1, 3), (0, 1, 40, 1500), (0, 1, 5, 29, 300, 1100), (0, 1, 3, 8, 9), (0, 1, 16, 128, 129)):
        add("e2e_gram_beam_max_width", V, K)
        add("e2e_gram_beam_workspace_bytes", B, T, V, K, W)
        for scored, lm in ((0, 0), (1, 0), (1, 1), (0, 1)):
            add("e2e_gram_beam_workspace_bytes_lm", B, T, V, K, W, lm)
            add("e2e_gram_beam_stream_row_bytes", T, V, K, W, scored, lm)
            add("e2e_gram_beam_stream_workspace_bytes", B, V, K, W, scored, lm)
    for B, T, V, W, lm in itertools.product((-1, 0, 1, 3), (0, 1, 40, 1500), (0, 1, 5, 29, 128, 129), (0, 1, 16, 128, 129), (0, 1)):
        add("e2e_asg_beam_max_width", V)
        add("e2e_asg_beam_workspace_bytes", B, T, V, W, lm)
        add("e2e_asg_beam_stream_row_bytes", T, V, W, lm)
        add("e2e_asg_beam_stream_workspace_bytes", B, V, W, lm)
    return {k: sorted(set(v)) for k, v in g.items()}


def run_queries(L):
    """{query name: [values]} in the order of query_grid()."""
    return {name: [int(getattr(L, name)(*a)) for a in rows] for name, rows in query_grid().items()}


# ---- the refused calls ----------------------------------------------------------------------------------------------------------
class Models:
    """The word-list models (e2e_lm_load_words: no file) the refused calls name, one per alphabet; `lex`: with the lexicon."""

    def __init__(self, L):
        self.L, self.made = L, {}

    def get(self, V, lex):
        if (V, lex) not in self.made:
            words = (C.c_char_p * 2)(b"ab", b"ba")
            labels = (C.c_char_p * V)(*[b"_", b" "] + [bytes([97 + i % 26]) * (1 + i // 26) for i in range(V - 2)])
            h = C.c_void_p()
            assert self.L.e2e_lm_load_words(words, 2, labels, V, 1, C.byref(h)) == 0
            if lex:
                assert self.L.e2e_lm_enable_lexicon(h) == 0
            self.made[(V, lex)] = h
        return self.made[(V, lex)]

    def free(self):
        for h in self.made.values():
            self.L.e2e_lm_free(h)
        self.made = {}


# Each entry point: the arguments of a call that passes every check but the last (the workspace is too small), then the steps
# of its checks IN THE ORDER THE ENTRY MAKES THEM, each with the changes that trip it alone.  lm: None, "words" (a word-list
# model of V labels without a lexicon) -- never one that passes the lexicon check, since the next thing such a call meets is
# whether the model's tables are on the device, which a machine without a GPU answers differently.
def _ctc_base(**kw):
    d = dict(lp=P, dtype=0, x_len=P, B=2, T=20, V=7, blank=0, W=10, space=-1, lm=None, nbest=10, out=P, max_out=21, out_len=P,
             n_hyp=P, scores=P, counts=P, timesteps=None, ws=P, ws_bytes=16, restrict=None, top_n=2, prob=1.0,
             state=P, row_bytes=None, max_frames=100, with_ts=0, frames_done=P)
    d.update(kw)
    return d


_CUT = [("cutoff_top_n", dict(top_n=0)), ("cutoff_prob", dict(prob=0.0))]
# (each step's change trips its check whatever the other arguments are, so that it stays live beside another step's change;
#  only two steps that are about one argument -- max_frames, the width, the state -- cannot both be live: the earlier one's value holds)
_WHOLE_TAIL = [("dtype", dict(dtype=9)), ("sizes", dict(T=0)), ("blank", dict(blank=-1)), ("null_lp", dict(lp=None))]
# (a stream has met T = 0 in its own sizes check long before: here the size that only the common check looks at)
_STREAM_TAIL = [("dtype", dict(dtype=9)), ("sizes", dict(max_out=0)), ("blank", dict(blank=-1)), ("null_lp", dict(lp=None))]
_NBEST = [("lexicon", dict(restrict=True)), ("nbest", dict(nbest=0)), ("null_nbest", dict(scores=None)), ("width", dict(W=513))]
_STREAM = [("stream_sizes", dict(max_frames=0)), ("nbest", dict(nbest=-1)), ("null_stream", dict(frames_done=None)),
           ("null_nbest", dict(counts=None)), ("timesteps", dict(timesteps=P)), ("width", dict(W=513)),
           ("max_frames", dict(max_frames=1 << 30)), ("row_bytes", dict(row_bytes=4096)),
           ("state_aligned", dict(state=P + 4)), ("lexicon", dict(restrict=True))]
_STREAM_BASE = dict(V=300, W=256, max_out=101)                           # (the general kernel: only it needs a workspace)

ENTRIES = {
    "e2e_ctc_beam": (_ctc_base(), _WHOLE_TAIL + [("width", dict(W=513)), ("workspace", dict())]),
    "e2e_ctc_beam_nbest": (_ctc_base(), _NBEST[1:] + _WHOLE_TAIL + [("workspace", dict())]),
    "e2e_ctc_beam_nbest_opt": (_ctc_base(restrict=False), _NBEST + _WHOLE_TAIL + [("workspace", dict())]),
    "e2e_ctc_beam_nbest_cut": (_ctc_base(restrict=False), _CUT + _NBEST + _WHOLE_TAIL +
                               [("cut_limit", dict(V=5000, top_n=2000, W=2, nbest=1)), ("workspace", dict())]),
    "e2e_ctc_beam_stream": (_ctc_base(restrict=False, **_STREAM_BASE), _STREAM + _STREAM_TAIL + [("workspace", dict())]),
    "e2e_ctc_beam_stream_cut": (_ctc_base(restrict=False, **_STREAM_BASE), _CUT + _STREAM + _STREAM_TAIL +
                                [("cut_limit", dict(V=5000, top_n=2000, W=2, nbest=1)), ("workspace", dict())]),
}
# single errors beyond the steps' own: what the CPU tests of the entry points try, and the other operand of each check
CTC_MORE = {
    "e2e_ctc_beam": [dict(B=-1), dict(V=0), dict(W=0), dict(max_out=0), dict(blank=-1), dict(x_len=None), dict(out=None), dict(out_len=None),
                     dict(ws=None), dict(W=513, V=8000), dict(W=600, V=29), dict(dtype=-1)],
    "e2e_ctc_beam_nbest": [dict(nbest=0), dict(nbest=-3), dict(out=None), dict(out_len=None), dict(n_hyp=None), dict(counts=None),
                           dict(W=513, nbest=1, V=29), dict(W=513, nbest=1, V=8000), dict(W=513, lm="words"), dict(W=0, nbest=0),
                           dict(V=0), dict(B=-1), dict(max_out=0)],
    "e2e_ctc_beam_nbest_opt": [dict(restrict=True, lm="words"), dict(restrict=None, nbest=0)],
    "e2e_ctc_beam_nbest_cut": [dict(prob=2.0), dict(prob=float("nan")), dict(top_n=-1), dict(nbest=5, W=4), dict(W=100000),
                               dict(V=5000, top_n=5000, prob=0.5, W=2, nbest=1), dict(top_n=7, prob=1.0, W=513), dict(top_n=7, prob=0.5, W=513),
                               dict(top_n=9, nbest=0), dict(restrict=True, lm="words")],
    "e2e_ctc_beam_stream": [dict(nbest=257), dict(T=0), dict(V=0), dict(W=0, nbest=0, row_bytes=4096), dict(B=-1), dict(state=None),
                            dict(x_len=None), dict(lp=None), dict(out=None), dict(out_len=None), dict(n_hyp=None), dict(scores=None),
                            dict(row_bytes="short"), dict(row_bytes="odd"), dict(with_ts=1, timesteps=P, row_bytes="no_ts"),
                            dict(V=7, W=513, nbest=1, row_bytes=1 << 20), dict(V=8000, W=513, nbest=1, row_bytes=1 << 20),
                            dict(restrict=True, lm="words"), dict(nbest=0, max_out=0), dict(nbest=0, out=None, ws=None),
                            dict(ws_bytes=16, ws=P), dict(max_out=0)],
    "e2e_ctc_beam_stream_cut": [dict(prob=1.5), dict(top_n=300, prob=1.0, ws=None), dict(top_n=300, prob=0.5, ws=None),
                                dict(row_bytes="short"), dict(nbest=0, top_n=0)],
}


def _opts(L_mod, kind, restrict, timesteps=None):
    if restrict is None:
        return None
    o = kind(int(bool(restrict))) if kind is L_mod.BeamOpts else kind(int(bool(restrict)), timesteps)
    return C.byref(o)


def call_ctc(L, L_mod, models, entry, a):
    lm = models.get(a["V"], False) if a["lm"] == "words" and a["V"] >= 2 else None
    head = (a["lp"], a["dtype"], a["T"] * a["V"], a["V"], 1, a["x_len"], a["B"], a["T"], a["V"], a["blank"], a["W"], a["space"], lm,
            1.0, 0.0, -10.0)
    nb = (a["nbest"], a["out"], a["max_out"], a["out_len"], a["n_hyp"], a["scores"], a["counts"], a["timesteps"])
    tail = (a["ws"], a["ws_bytes"], None)
    opts = _opts(L_mod, L_mod.BeamOpts, a["restrict"])
    cut = (a["top_n"], a["prob"])
    if entry == "e2e_ctc_beam":
        return L.e2e_ctc_beam(*head, a["out"], a["max_out"], a["out_len"], *tail)
    if entry == "e2e_ctc_beam_nbest":
        return L.e2e_ctc_beam_nbest(*head, *nb, *tail)
    if entry == "e2e_ctc_beam_nbest_opt":
        return L.e2e_ctc_beam_nbest_opt(*head, *nb, *tail, opts)
    if entry == "e2e_ctc_beam_nbest_cut":
        return L.e2e_ctc_beam_nbest_cut(*head, *nb, *tail, opts, *cut)
    rb = a["row_bytes"]
    if rb is None or isinstance(rb, str):
        want = L.e2e_ctc_beam_stream_row_bytes(a["max_frames"], a["V"], a["W"], lm is not None, 0 if rb == "no_ts" else a["with_ts"])
        rb = want + {None: 0, "no_ts": 0, "short": -256, "odd": 4}[rb]
    st = (a["state"], rb, a["max_frames"], a["with_ts"])
    if entry == "e2e_ctc_beam_stream":
        return L.e2e_ctc_beam_stream(*head, *st, *nb, a["frames_done"], *tail, opts)
    assert entry == "e2e_ctc_beam_stream_cut", entry
    return L.e2e_ctc_beam_stream_cut(*head, *st, *nb, a["frames_done"], *tail, opts, *cut)


# ---- Gram-CTC and ASG: the n-best and stream entries ----
def _gram_base(**kw):
    d = dict(lp=P, dtype=0, x_len=P, B=2, T=20, V=7, gram_ids=P, gram_len=P, K=2, R=4, W=10, scored=1, space=-1, lm=None, nbest=10, out=P,
             max_out=41, out_len=P, n_hyp=P, scores=P, counts=P, ws=P, ws_bytes=16, restrict=None, timesteps=None, state=P,
             row_bytes=None, max_frames=100, frames_done=P)
    d.update(kw)
    return d


_GRAM_ARGS = [("dtype", dict(dtype=2)), ("sizes", dict(T=0)), ("max_order", dict(K=9)), ("width_low", dict(W=0)), ("width_max", dict(W=129)),
              ("nbest", dict(nbest=11))]
_GRAM_SCORED = [("base_labels", dict(R=8)), ("space", dict(space=4)), ("lexicon", dict(restrict=True))]
GRAM_ENTRIES = {
    "e2e_gram_ctc_beam_nbest": (_gram_base(), _GRAM_ARGS + [("frames", dict(T=1 << 23)), ("null", dict(gram_len=None)), ("workspace", dict())]),
    "e2e_gram_ctc_beam_nbest_lm": (_gram_base(), _GRAM_ARGS + _GRAM_SCORED[:2] + [("frames", dict(T=1 << 23)), ("null", dict(counts=None)),
                                                                                  ("workspace", dict())]),
    "e2e_gram_ctc_beam_nbest_opt": (_gram_base(restrict=False), _GRAM_ARGS + _GRAM_SCORED + [("frames", dict(T=1 << 23)), ("null", dict(out=None)),
                                                                                             ("workspace", dict())]),
    "e2e_gram_ctc_beam_stream": (_gram_base(restrict=False), _GRAM_ARGS[:5] + [("nbest", dict(nbest=-1))] + _GRAM_SCORED +
                                 [("max_frames", dict(max_frames=0, row_bytes=4096)), ("row_bytes", dict(row_bytes=4096)),
                                  ("null", dict(state=None)), ("null_out", dict(n_hyp=None)), ("state_aligned", dict(state=P + 4)),
                                  ("workspace", dict())]),
}
GRAM_MORE = {
    "e2e_gram_ctc_beam_nbest": [dict(B=-1), dict(max_out=-1), dict(K=0), dict(nbest=0), dict(lp=None), dict(scores=None), dict(out=None), dict(ws=None)],
    "e2e_gram_ctc_beam_nbest_lm": [dict(R=0), dict(lm="words")],
    "e2e_gram_ctc_beam_nbest_opt": [dict(restrict=True, lm="words"), dict(lm="words"), dict(counts=None), dict(n_hyp=None)],
    "e2e_gram_ctc_beam_stream": [dict(scored=0), dict(scored=0, restrict=None), dict(scored=0, restrict=None, counts=None, R=0), dict(row_bytes="odd"),
                                 dict(row_bytes="short"), dict(max_frames=(1 << 22) + 1, row_bytes=1 << 20), dict(frames_done=None),
                                 dict(nbest=0, out_len=None), dict(counts=None), dict(restrict=True, lm="words"), dict(nbest=0, max_out=-1)],
}


def call_gram(L, L_mod, models, entry, a):
    lm = models.get(a["R"], False) if a["lm"] == "words" and a["R"] >= 2 else None
    x = (a["lp"], a["dtype"], a["T"] * a["V"], a["V"], 1, a["x_len"], a["B"], a["T"], a["V"], a["gram_ids"], a["gram_len"], a["K"])
    out = (a["nbest"], a["out"], a["max_out"], a["out_len"], a["n_hyp"], a["scores"])
    tail = (a["ws"], a["ws_bytes"], None)
    opts = _opts(L_mod, L_mod.GramBeamOpts, a["restrict"], a["timesteps"])
    if entry == "e2e_gram_ctc_beam_nbest":
        return L.e2e_gram_ctc_beam_nbest(*x, a["W"], *out, *tail)
    scored = (a["R"], a["W"], a["space"], lm, 1.0, 0.0, -10.0)
    if entry == "e2e_gram_ctc_beam_nbest_lm":
        return L.e2e_gram_ctc_beam_nbest_lm(*x, *scored, *out, a["counts"], *tail)
    if entry == "e2e_gram_ctc_beam_nbest_opt":
        return L.e2e_gram_ctc_beam_nbest_opt(*x, *scored, *out, a["counts"], *tail, opts)
    assert entry == "e2e_gram_ctc_beam_stream", entry
    rb = a["row_bytes"]
    if rb is None or isinstance(rb, str):
        rb = L.e2e_gram_beam_stream_row_bytes(a["max_frames"], a["V"], a["K"], a["W"], a["scored"], lm is not None) + {None: 0, "short": -256, "odd": 4}[rb]
    return L.e2e_gram_ctc_beam_stream(*x, a["R"], a["W"], a["scored"], a["space"], lm, 1.0, 0.0, -10.0, a["state"], rb, a["max_frames"],
                                      *out, a["counts"], a["frames_done"], *tail, opts)


def _asg_base(**kw):
    d = dict(x=P, dtype=0, trans=P, x_len=P, B=2, T=20, V=7, reps=1, W=10, space=-1, lm=None, nbest=10, out=P, max_out=21, out_len=P,
             n_hyp=P, scores=P, counts=P, ws=P, ws_bytes=16, restrict=None, timesteps=None, state=P, row_bytes=None, max_frames=100,
             frames_done=P)
    d.update(kw)
    return d


_ASG_ARGS = [("dtype", dict(dtype=2)), ("sizes", dict(T=0)), ("labels", dict(V=129)), ("replabels", dict(reps=7)), ("space", dict(space=6)),
             ("width_low", dict(W=0)), ("width_max", dict(W=129)), ("nbest", dict(nbest=11))]
ASG_ENTRIES = {
    "e2e_asg_beam_nbest": (_asg_base(), _ASG_ARGS + [("frames", dict(T=1 << 23)), ("null", dict(n_hyp=None)), ("workspace", dict())]),
    "e2e_asg_beam_nbest_opt": (_asg_base(restrict=False), _ASG_ARGS + [("frames", dict(T=1 << 23)), ("lexicon", dict(restrict=True)),
                                                                       ("null", dict(x=None)), ("workspace", dict())]),
    "e2e_asg_beam_stream": (_asg_base(restrict=False), _ASG_ARGS[:7] + [("nbest", dict(nbest=-1)), ("max_frames", dict(max_frames=0, row_bytes=4096)),
                                                                        ("row_bytes", dict(row_bytes=4096)), ("lexicon", dict(restrict=True)),
                                                                        ("null", dict(frames_done=None)), ("null_out", dict(counts=None)),
                                                                        ("state_aligned", dict(state=P + 4)), ("workspace", dict())]),
}
ASG_MORE = {
    "e2e_asg_beam_nbest": [dict(B=-1), dict(max_out=-1), dict(reps=-1), dict(nbest=0), dict(x_len=None), dict(out=None), dict(ws=None)],
    "e2e_asg_beam_nbest_opt": [dict(restrict=True, lm="words"), dict(scores=None)],
    "e2e_asg_beam_stream": [dict(row_bytes="odd"), dict(row_bytes="short"), dict(max_frames=(1 << 22) + 1, row_bytes=1 << 20), dict(state=None),
                            dict(nbest=0, out_len=None), dict(restrict=True, lm="words"), dict(nbest=0, max_out=-1), dict(lm="words", V=8)],
}


def call_asg(L, L_mod, models, entry, a):
    lm = models.get(a["V"], False) if a["lm"] == "words" and a["V"] >= 2 else None
    head = (a["x"], a["dtype"], a["T"] * a["V"], a["V"], 1, a["trans"], a["x_len"], a["B"], a["T"], a["V"], a["reps"], a["W"], a["space"],
            lm, 1.0, 0.0, -10.0)
    out = (a["nbest"], a["out"], a["max_out"], a["out_len"], a["n_hyp"], a["scores"], a["counts"])
    tail = (a["ws"], a["ws_bytes"], None)
    opts = _opts(L_mod, L_mod.AsgBeamOpts, a["restrict"], a["timesteps"])
    if entry == "e2e_asg_beam_nbest":
        return L.e2e_asg_beam_nbest(*head, *out, *tail)
    if entry == "e2e_asg_beam_nbest_opt":
        return L.e2e_asg_beam_nbest_opt(*head, *out, *tail, opts)
    assert entry == "e2e_asg_beam_stream", entry
    rb = a["row_bytes"]
    if rb is None or isinstance(rb, str):
        rb = L.e2e_asg_beam_stream_row_bytes(a["max_frames"], a["V"], a["W"], lm is not None) + {None: 0, "short": -256, "odd": 4}[rb]
    return L.e2e_asg_beam_stream(*head, a["state"], rb, a["max_frames"], *out, a["frames_done"], *tail, opts)


# what each step's own error says: the single call reports it, and so does every pair in which the step comes first
EXPECT = {"cutoff_top_n": "cutoff_top_n=", "cutoff_prob": "cutoff_prob=", "lexicon": "restrict_to_lexicon", "nbest": "nbest=",
          "null_nbest": "null pointer", "width": "over an alphabet", "width_max": "exceeds e2e_",
          "dtype": "dtype must be", "sizes": "bad sizes", "blank": "blank=",
          "null_lp": "null pointer", "cut_limit": "cutoff_top_n", "workspace": "workspace too small", "stream_sizes": "bad sizes",
          "null_stream": "null pointer", "timesteps": "timesteps asked", "max_frames": "max_frames", "row_bytes": "row_bytes =",
          "state_aligned": "8-byte aligned", "max_order": "max_order", "width_low": "must be at least 1", "frames": "frames are more",
          "null": "null pointer", "null_out": "null pointer", "base_labels": "num_base_labels", "space": "space_id",
          "labels": "e2e_asg_max_labels", "replabels": "num_replabels"}
# pairs further apart than three places that the entry points' definition names
FAR_PAIRS = {"e2e_ctc_beam_nbest_cut": [("cutoff_prob", "blank"), ("cutoff_top_n", "blank"), ("cutoff_prob", "workspace")],
             "e2e_ctc_beam_stream_cut": [("cutoff_prob", "blank"), ("cutoff_top_n", "blank"), ("cutoff_prob", "workspace")]}

FAMILIES = ((ENTRIES, CTC_MORE, call_ctc), (GRAM_ENTRIES, GRAM_MORE, call_gram), (ASG_ENTRIES, ASG_MORE, call_asg))


def refused_calls():
    """[(case id, call function, entry, arguments)]: per entry every step alone, the further single errors, and every two steps
    that are at most three places apart in the entry's order, tripped together, and the FAR_PAIRS."""
    cases = []
    for entries, more, call in FAMILIES:
        for entry, (base, steps) in entries.items():
            for name, change in steps:
                cases.append(("%s/%s" % (entry, name), call, entry, dict(base, **change)))
            for i, change in enumerate(more.get(entry, ())):
                cases.append(("%s/more%d" % (entry, i), call, entry, dict(base, **change)))
            for gap in (1, 2, 3):
                for (n1, c1), (n2, c2) in zip(steps, steps[gap:]):
                    # (the later step's changes first: where both set one argument, the earlier step's value trips the earlier check)
                    cases.append(("%s/%s+%s" % (entry, n1, n2), call, entry, dict(base, **dict(c2, **c1))))
            for n1, n2 in FAR_PAIRS.get(entry, ()):
                cases.append(("%s/%s+%s" % (entry, n1, n2), call, entry, dict(base, **dict(dict(steps)[n2], **dict(steps)[n1]))))
    assert len({c[0] for c in cases}) == len(cases)
    return cases


def run_refused(L, L_mod):
    """{case id: [return code, e2e_last_error()]}; no call may succeed."""
    models = Models(L)
    got = {}
    try:
        for cid, call, entry, args in refused_calls():
            rc = call(L, L_mod, models, entry, args)
            assert rc != 0, "%s was not refused" % cid
            got[cid] = [int(rc), L.e2e_last_error().decode()]
    finally:
        models.free()
    return got
