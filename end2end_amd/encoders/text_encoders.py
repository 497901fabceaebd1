"""Text <-> label-id helpers (host-side): CTCEncoder with the behaviour of the reference's
(pytorch_end2end/encoders/text_encoders.py:8-41), and ASGEncoder, which upstream declares (text_encoders.py:44-51) and
leaves at NotImplementedError."""
import string

import numpy as np


class CTCEncoder:
    """Maps characters to consecutive ids, leaving `blank_id` free for the CTC blank."""

    def __init__(self, characters, blank_id=0, transform_fn=str.upper):
        self.blank_id = blank_id
        self.transform_fn = transform_fn
        self.char2id = {}
        next_id = 0
        for ch in characters:
            if next_id == blank_id:
                next_id += 1            # skip over the blank's slot
            self.char2id[ch] = next_id
            next_id += 1
        self.id2char = {i: ch for ch, i in self.char2id.items()}
        self.id2char[blank_id] = ""
        self.num_symbols = len(self.id2char)

    def _known(self, text):
        return [ch for ch in self.transform_fn(text) if ch in self.char2id]

    def clean(self, text):
        return "".join(self._known(text))

    def encode(self, text):
        return np.array([self.char2id[ch] for ch in self._known(text)])

    def decode(self, ids_list):
        """Collapse repeats, drop blanks."""
        out, prev = [], object()
        for i in ids_list:
            if i != prev and i != self.blank_id:
                out.append(self.id2char[i])
            prev = i
        return "".join(out)

    def decode_pure(self, ids_list):
        return "".join(self.id2char[i] for i in ids_list)


class ASGEncoder:
    """
    Encoder for the Auto Segmentation Criterion (http://arxiv.org/abs/1609.03193) and CTC without blank: there is no
    blank, so a doubled letter is spelled with a repeat label, as wav2letter does.  Characters get ids from 0 in the given
    order; repeat label ``r`` (``1 <= r <= num_replabels``), "the character before, ``r`` more times", is
    ``len(allowed_chars) + r - 1``.

    :param allowed_chars: the alphabet; other characters are dropped
    :param to_lower: case folding applied before anything else
    :param num_replabels: R, the number of repeat labels (upstream's signature has none; 0: runs are merged, since a
        blank-free model without repeat labels cannot spell them)
    """

    def __init__(self, allowed_chars=" " + string.ascii_lowercase + "'", to_lower=str.casefold, num_replabels=2):
        if int(num_replabels) < 0:
            raise ValueError("num_replabels must be >= 0")
        self.to_lower = to_lower
        self.num_replabels = int(num_replabels)
        self.char2id = {}
        for ch in allowed_chars:
            self.char2id.setdefault(ch, len(self.char2id))
        self.id2char = {i: ch for ch, i in self.char2id.items()}
        self.num_chars = len(self.char2id)
        self.num_symbols = self.num_chars + self.num_replabels

    def replabel_id(self, r):
        return self.num_chars + r - 1

    def _known(self, text):
        return [ch for ch in self.to_lower(text) if ch in self.char2id]

    def clean(self, text):
        """The text as the ids can spell it: case folded, unknown characters dropped -- and, without repeat labels, runs
        of one character merged."""
        chars = self._known(text)
        if self.num_replabels == 0:
            chars = [ch for i, ch in enumerate(chars) if i == 0 or ch != chars[i - 1]]
        return "".join(chars)

    def encode(self, text):
        """Runs are packed as wav2letter packs them: the character, then -- if the run goes on -- the repeat label of
        min(run - 1, R), then on behind what that consumed.  hello -> h e l <1> o; R = 2: aaaa -> a <2> a.  No two equal
        ids are ever adjacent."""
        chars = list(self.clean(text))
        R, out, i = self.num_replabels, [], 0
        while i < len(chars):
            run = 1
            while i + run < len(chars) and chars[i + run] == chars[i]:
                run += 1
            out.append(self.char2id[chars[i]])
            rep = min(run - 1, R)
            if rep > 0:
                out.append(self.replabel_id(rep))
            i += 1 + rep
        return np.array(out, dtype=np.int64)

    def decode(self, ids_list):
        """Merge consecutive repeats (a frame path becomes a label sequence), then expand the repeat labels; a leading
        one has nothing to repeat and is dropped, as are negative (padding) ids."""
        out, prev = [], object()
        for i in ids_list:
            i = int(i)
            if i == prev or i < 0:
                prev = i
                continue
            prev = i
            if i < self.num_chars:
                out.append(self.id2char[i])
            elif i < self.num_symbols:
                if out:
                    out.extend(out[-1] * (i - self.num_chars + 1))
            else:
                raise KeyError(i)
        return "".join(out)

    def decode_pure(self, ids_list):
        """Id by id, nothing merged or expanded: a repeat label shows as its digit(s)."""
        return "".join(self.id2char[int(i)] if int(i) < self.num_chars else str(int(i) - self.num_chars + 1)
                       for i in ids_list)
