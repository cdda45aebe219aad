"""Label <-> string helpers (reference: utils/string_utils.py, utils/error_rates.py)."""
import numpy as np


def str2label_single(value, characterToIndex, unknown_index=None):
    return np.array([characterToIndex[v] for v in value if v in characterToIndex], np.uint32)


def label2str_single(label, indexToCharacter, asRaw, spaceChar="~"):
    out = ""
    for v in label:
        if v == 0:
            if not asRaw:
                break
            out += spaceChar
        else:
            out += indexToCharacter[v]
    return out


def naive_decode(output):
    """greedy CTC decode of [T, C] scores: collapse repeats, drop blanks"""
    raw = np.argmax(output, axis=1)
    pred = [raw[i] for i in range(len(raw)) if raw[i] != 0 and not (i > 0 and raw[i] == raw[i - 1])]
    return pred, list(raw)


def _levenshtein(a, b):
    prev = list(range(len(b) + 1))
    for i, ca in enumerate(a, 1):
        cur = [i]
        for j, cb in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (ca != cb)))
        prev = cur
    return prev[-1]


def cer(r, h, casesensitive=True):
    r, h = " ".join(r.split()), " ".join(h.split())
    if not casesensitive:
        r, h = r.lower(), h.lower()
    if len(r) == 0:
        return len(h)
    return _levenshtein(r, h) / float(len(r))


def wer(r, h, casesensitive=True):
    if not casesensitive:
        r, h = r.lower(), h.lower()
    r, h = r.split(), h.split()
    if len(r) == 0:
        return len(h)
    return _levenshtein(r, h) / float(len(r))


def prefix_beam_decode(lp, beam):
    """CTC prefix beam search over [T, C] log-probabilities as they stand (class 0 the blank, a NaN reads as -inf), in fp64: the host side
    and definition of ops.ctc_beam_error_rates (csrc/ctc_beam.hip). -> (ids, score, totals): the prefix of largest total (pb (+) pnb, (+) =
    log-add-exp), that total (-inf with an empty beam, ids [] then), and all final totals, descending, padded with -inf to `beam`.
    Of exactly equal totals the candidate of the earlier beam slot wins, within a slot the prefix itself before its extensions in ascending
    class order - the kernel's rule."""
    lp = np.array(lp, dtype=np.float64)
    lp[np.isnan(lp)] = -np.inf
    T, C = lp.shape
    ninf = -np.inf
    lse = np.logaddexp
    slots = [((), 0.0, ninf)]                            # (prefix, pb, pnb), best first
    with np.errstate(invalid="ignore"):
        for t in range(T):
            row = lp[t]
            new = {}                                     # prefix -> [pb, pnb, candidate index]
            for j, (pre, pb, pnb) in enumerate(slots):
                new[pre] = [ninf, ninf, j * C]
            for j, (pre, pb, pnb) in enumerate(slots):
                tot = lse(pb, pnb)
                e = new[pre]
                e[0] = lse(e[0], row[0] + tot)
                if pre:
                    e[1] = lse(e[1], row[pre[-1]] + pnb)
                for c in range(1, C):
                    v = row[c] + (pb if pre and c == pre[-1] else tot)
                    if v == ninf:
                        continue
                    e = new.get(pre + (c,))
                    if e is None:
                        new[pre + (c,)] = [ninf, v, j * C + c]
                    else:
                        e[1] = lse(e[1], v)
            cand = [(lse(pb, pnb), idx, pre, pb, pnb) for pre, (pb, pnb, idx) in new.items()]
            cand = sorted((x for x in cand if x[0] > ninf), key=lambda x: (-x[0], x[1]))[:beam]
            slots = [(pre, pb, pnb) for _, _, pre, pb, pnb in cand]
    totals = np.full(beam, ninf)
    totals[:len(slots)] = [lse(pb, pnb) for _, pb, pnb in slots]
    if not slots:
        return [], ninf, totals
    return list(slots[0][0]), float(totals[0]), totals


def shortest_ctc_path(ids, T):
    """the shortest CTC alignment of the class sequence `ids`: one blank between equal neighbours, zero padded to T frames (what the beam
    kernel hands to the greedy collapse, which returns exactly `ids`); ValueError when it does not fit"""
    path = []
    for i, c in enumerate(ids):
        if i and c == ids[i - 1]:
            path.append(0)
        path.append(int(c))
    if len(path) > T:
        raise ValueError("a text of %d classes with %d doubled neighbours has no alignment of %d frames" % (len(ids), len(path) - len(ids), T))
    return path + [0] * (T - len(path))


# ---- the host side of ops.ctc_error_rates: cer / wer above, split into what the host prepares, what the device counts and the division ----
SPACE = 32


def normalise_ref(text, casesensitive=True):
    """the reference side of cer / wer -> its code points: " ".join(text.split()), lower-cased as a whole when the comparison ignores case
    (words of it are the runs between single spaces: text.lower().split() gives the same words)"""
    text = " ".join(text.split())
    if not casesensitive:
        text = text.lower()
    return [ord(ch) for ch in text]


def class_code_table(idx_to_char, num_class, casesensitive=True):
    """-> int32 [num_class]: the code point class c compares as - 32 for every character str.split() splits at, the lower-cased character
    when the comparison ignores case; entry 0 (the CTC blank) is unused. None when comparing class by class would not be cer / wer of the
    decoded string whatever the case switch says: a class without exactly one character, one whose lower-casing is not exactly one character
    (such as 'İ'), or 'Σ', which str.lower() turns into 'σ' or 'ς' depending on where in a word it stands."""
    table = np.zeros(num_class, dtype=np.int32)
    for c in range(1, num_class):
        ch = idx_to_char.get(c)
        if not isinstance(ch, str) or len(ch) != 1:
            return None
        if ch == "Σ" or len(ch.lower()) != 1:
            return None
        if not casesensitive:
            ch = ch.lower()
        table[c] = SPACE if ch.isspace() else ord(ch)
    return table


def rates_from_counts(dist, ref_len, hyp_len):
    """cer (or, on words, wer) from the integers the device counts: the edit distance over the reference's length, or the hypothesis's length
    when the reference is empty - the same Python arithmetic as cer / wer, so the same bits"""
    if ref_len == 0:
        return hyp_len
    return dist / float(ref_len)
