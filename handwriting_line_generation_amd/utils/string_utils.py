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
