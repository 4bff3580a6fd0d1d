"""Pure-Python restatement of the n-gram rule of include/loco_asr.h (csrc/ngram.hip, loco-asr_amd/ngram.py): a dict-based
interpolated Witten-Bell trainer in backoff form, an ARPA reader and writer, and the backoff scorer.  Nothing here shares code with the
product.  A model is ``Model(order, V, logp, bo)``: ``logp[gram]`` and ``bo[gram]`` are natural logarithms keyed by tuples of symbols,
oldest first; predicted symbols are 0 .. V - 1 (2 is </s>), contexts may open with BOS = V; the unigram ``(V,)`` carries bo of <s>."""
import math
from collections import namedtuple
from fractions import Fraction

import numpy as np

EOS = 2
LN10 = math.log(10.0)
BOS_LOG10 = -99.0  # ARPA's conventional log10 P(<s>): the gram is a context only

Model = namedtuple("Model", "order V logp bo")


def sentences(seqs, V):
    return [[V] + [int(t) for t in s] + [EOS] for s in seqs]


def wb_probabilities(seqs, order, V, exact=False):
    """({gram: P(w | h)}, {context: bo(h)}) of the seen grams by P_j(w|h) = (c(hw) + T(h) P_{j-1}(w|h')) / (c(h) + T(h)), P_0 = 1/V,
    bo(h) = T(h) / (c(h) + T(h)); as Fractions with ``exact``.  Every id has a unigram; a context that is no gram's prefix has no bo."""
    num = (lambda a, b: Fraction(a, b)) if exact else (lambda a, b: a / b)
    count = {}
    for s in sentences(seqs, V):
        for i in range(1, len(s)):
            for j in range(order):
                if i - j < 0:
                    break
                g = tuple(s[i - j:i + 1])
                count[g] = count.get(g, 0) + 1
    total, types = {}, {}
    for g, c in count.items():
        total[g[:-1]] = total.get(g[:-1], 0) + c
        types[g[:-1]] = types.get(g[:-1], 0) + 1
    assert total.get((), 0) > 0, "an empty corpus"
    bo = {h: num(types[h], total[h] + types[h]) for h in total}
    prob = {}

    def p(g):
        """P(w | h) for any gram, seen or not"""
        if g in prob:
            return prob[g]
        h = g[:-1]
        if len(g) == 1:
            lower = num(1, V)
        else:
            lower = p(g[1:])
        if h not in total:
            return lower
        v = (count.get(g, 0) + types[h] * lower) / (total[h] + types[h])
        if g in count or len(g) == 1:
            prob[g] = v
        return v

    for w in range(V):
        p((w,))
    for g in sorted(count, key=len):
        p(g)
    return prob, bo


def train(seqs, order, V):
    prob, bo = wb_probabilities(seqs, order, V)
    logp = {g: math.log(v) for g, v in prob.items()}
    logp[(V,)] = BOS_LOG10 * LN10
    lbo = {g: 0.0 for g in logp}
    for h, v in bo.items():
        if h:  # the empty context's weight is inside the unigrams
            lbo[h] = math.log(v)
    return Model(order, V, logp, lbo)


def logprob(model, history, w):
    """The chain: ``history`` is the row's symbols so far (index 0 already BOS)."""
    m = min(model.order - 1, len(history))
    h = tuple(history[len(history) - m:])
    acc = 0.0
    for j in range(m, -1, -1):
        ctx = h[m - j:]
        if ctx + (w,) in model.logp:
            return acc + model.logp[ctx + (w,)]
        if j > 0 and ctx in model.logp:
            acc = acc + model.bo[ctx]
    raise KeyError(f"no unigram for {w}")


def symbols_of(row, V):
    """A token row (index 0 the start token) as the rule's symbols."""
    return [V] + [int(t) for t in row[1:]]


def next_logprobs(model, row):
    """float64 [V]: log P(w | row) for every w; ``row`` holds the tokens so far, index 0 the start token."""
    h = symbols_of(row, model.V)
    return np.array([logprob(model, h, w) for w in range(model.V)], dtype=np.float64)


def token_logprobs(model, seq):
    """float64 [len]: entry i = log P(seq[i] | seq[:i]), entry 0 = 0."""
    h = symbols_of(seq, model.V)
    return np.array([0.0] + [logprob(model, h[:i], int(seq[i])) for i in range(1, len(seq))], dtype=np.float64)


def word_of(sym, V):
    return "<s>" if sym == V else "</s>" if sym == EOS else str(sym)


def write_arpa(model, path):
    by_len = {}
    for g in model.logp:
        by_len.setdefault(len(g), []).append(g)
    with open(path, "w") as f:
        f.write("\\data\\\n")
        for n in sorted(by_len):
            f.write(f"ngram {n}={len(by_len[n])}\n")
        for n in sorted(by_len):
            f.write(f"\n\\{n}-grams:\n")
            for g in sorted(by_len[n]):
                words = " ".join(word_of(s, model.V) for s in g)
                tail = "" if model.bo[g] == 0.0 else "\t%.17g" % (model.bo[g] / LN10)
                f.write("%.17g\t%s%s\n" % (model.logp[g] / LN10, words, tail))
        f.write("\n\\end\\\n")


def read_arpa(path, V):
    logp, bo, order, section = {}, {}, 0, 0
    unk = None
    for line in open(path):
        line = line.strip()
        if not line or line == "\\data\\" or line.startswith("ngram "):
            continue
        if line == "\\end\\":
            break
        if line.startswith("\\") and line.endswith("-grams:"):
            section = int(line[1:line.index("-")])
            order = max(order, section)
            continue
        parts = line.split()
        words = parts[1:1 + section]
        if words == ["<unk>"]:
            unk = float(parts[0]) * LN10
            continue
        g = []
        for w in words:
            if w == "2":
                raise ValueError("the word '2' beside </s>")
            g.append(V if w == "<s>" else EOS if w == "</s>" else int(w))
        g = tuple(g)
        logp[g] = float(parts[0]) * LN10
        bo[g] = float(parts[1 + section]) * LN10 if len(parts) > 1 + section else 0.0
    for w in range(V):
        if (w,) not in logp:
            if unk is None:
                raise ValueError(f"no unigram for {w} and no <unk>")
            logp[(w,)], bo[(w,)] = unk, 0.0
    return Model(order, V, logp, bo)


def arrays(model):
    """(lengths i32 [n], symbols i32 [n, 8], logp f64 [n], backoff f64 [n]) of loco_ngram_create, grams in sorted order."""
    grams = sorted(model.logp, key=lambda g: (len(g), g))
    lengths = np.array([len(g) for g in grams], np.int32)
    symbols = np.zeros((len(grams), 8), np.int32)
    for i, g in enumerate(grams):
        symbols[i, :len(g)] = g
    return lengths, symbols, np.array([model.logp[g] for g in grams], np.float64), np.array([model.bo[g] for g in grams], np.float64)


def corpus(seed, sentences_n, ids, length=(3, 12), V=None):
    """Seeded sequences over ``ids`` with some structure (a random bigram chain), without specials."""
    rng = np.random.default_rng(seed)
    ids = list(ids)
    nxt = {a: rng.choice(ids, size=3) for a in ids}
    out = []
    for _ in range(sentences_n):
        n = int(rng.integers(length[0], length[1] + 1))
        s = [int(rng.choice(ids))]
        while len(s) < n:
            s.append(int(rng.choice(nxt[s[-1]])) if rng.random() < 0.8 else int(rng.choice(ids)))
        out.append(s)
    return out
