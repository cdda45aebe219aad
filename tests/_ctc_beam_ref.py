"""CTC prefix beam search restated as a dictionary loop over tuples (not collected by pytest): the reference of tests/test_ctc_beam_*.py,
written independently of string_utils.prefix_beam_decode. dtype = float64 is the reference; dtype = float32 is the same loop in numpy
float32, the yardstick of what fp32 arithmetic can deliver on a case.

Definition (include/hwg.h, hwg_ctc_beam_error_rates): lp [T, C] log-probabilities as they stand, class 0 the blank, NaN = -inf. A beam of at
most K prefixes with pb / pnb, tot = pb (+) pnb; start {(): (0, -inf)}. Per frame, for every beam prefix l into a fresh table (entries
made as (-inf, -inf)):  new[l].pb (+)= lp[0] + tot(l);  l not empty: new[l].pnb (+)= lp[last(l)] + pnb(l);  every c >= 1:
new[l + c].pnb (+)= lp[c] + (pb(l) if c == last(l) else tot(l)). The new beam: the K entries of largest finite tot.
The order among exactly equal totals is the table's insertion order here (a stable sort); the tests compare texts of decided cases only."""
import numpy as np

# (probabilities [T][C], beam, text, probability of the text, greedy text)
HAND_CASES = [
    # greedy scores the one alignment (blank, blank) = 0.36; "a" sums a-, -a, aa = 0.24 + 0.24 + 0.16
    ([[.6, .4], [.6, .4]], 4, [1], 0.64, []),
    # a doubled letter needs the blank between: "aa" has the one alignment a-a = 0.9 * 0.8 * 0.9 = 0.648; "a" collects a--, -a-, --a, aa-,
    # -aa, aaa = 0.072 + 0.002 + 0.072 + 0.018 + 0.018 + 0.162 = 0.344, the empty text --- = 0.008
    ([[.1, .9], [.8, .2], [.1, .9]], 4, [1, 1], 0.648, [1, 1]),
]


def search(lp, K, dtype=np.float64):
    """-> dict: text (tuple), score, totals [K] (descending, -inf padded), and - meant for the float64 run -
    gap: the smallest decision gap: over all frames tot of the K-th kept minus tot of the best dropped finite entry, at the end best minus
         second (inf where nothing finite was dropped / there is no second);
    reentries: prefixes entering the beam that had been in it before and were not in it the frame before;
    trap: those of them of which an extension by one class was in the beam the frame before (the case a second trie node would break)"""
    lp = np.array(lp, dtype=dtype)
    lp[np.isnan(lp)] = -np.inf
    T, C = lp.shape
    ninf = dtype(-np.inf)
    beam = {(): (dtype(0), ninf)}
    seen = {()}
    gap, reentries, trap = np.inf, 0, 0
    with np.errstate(invalid="ignore"):
        for t in range(T):
            row = lp[t]
            new = {}
            for pre, (pb, pnb) in beam.items():
                tot = np.logaddexp(pb, pnb)
                e = new.setdefault(pre, [ninf, ninf])
                e[0] = np.logaddexp(e[0], row[0] + tot)
                last = pre[-1] if pre else 0
                if pre:
                    e[1] = np.logaddexp(e[1], row[last] + pnb)
                ext = row + tot                                          # one vector add per prefix: the same dtype, the same values
                if pre:
                    ext[last] = row[last] + pb
                for c in range(1, C):
                    e = new.setdefault(pre + (c,), [ninf, ninf])
                    e[1] = np.logaddexp(e[1], ext[c])
            keys = list(new)
            tots = np.logaddexp(np.array([new[k][0] for k in keys], dtype=dtype), np.array([new[k][1] for k in keys], dtype=dtype))
            finite = np.flatnonzero(tots > ninf)
            order = finite[np.argsort(-tots[finite], kind="stable")]
            if len(order) > K:
                gap = min(gap, float(tots[order[K - 1]]) - float(tots[order[K]]))
            kept = [keys[i] for i in order[:K]]
            for pre in kept:
                if pre in seen and pre not in beam:
                    reentries += 1
                    trap += any(len(q) == len(pre) + 1 and q[:-1] == pre for q in beam)
            seen.update(kept)
            beam = {pre: (new[pre][0], new[pre][1]) for pre in kept}
    totals = np.full(K, -np.inf, dtype=dtype)
    texts = list(beam)
    totals[:len(texts)] = [np.logaddexp(*beam[p]) for p in texts]
    if len(texts) > 1:
        gap = min(gap, float(totals[0]) - float(totals[1]))
    return dict(text=texts[0] if texts else (), score=dtype(totals[0]), totals=totals, gap=gap, reentries=reentries, trap=trap)


def shortest_path(text, T):
    """the shortest CTC alignment of `text`: one blank between equal neighbours, zero padded to T (None when it does not fit)"""
    path = []
    for i, c in enumerate(text):
        if i and c == text[i - 1]:
            path.append(0)
        path.append(int(c))
    return path + [0] * (T - len(path)) if len(path) <= T else None


def log_softmax_rows(T, C, sigma, seed):
    """log-softmax of sigma * N(0, 1) rows, fp32 [T, C] (computed in fp64, rounded once)"""
    x = sigma * np.random.RandomState(seed).randn(T, C)
    x -= x.max(axis=1, keepdims=True)
    return (x - np.log(np.exp(x).sum(axis=1, keepdims=True))).astype(np.float32)
