"""What the n-gram and shallow-fusion tests share: the contexts every model is probed with and the model the fused beam search uses."""
import ngram_ref

V_MODEL = 81
LM_ORDER, LM_WEIGHT, LM_BONUS = 3, 1.0, 0.3
SEEN_IDS = range(4, 24)  # the ids the corpora are drawn from; ids from 24 on are never seen


def fusion_corpus():
    return ngram_ref.corpus(7, 300, SEEN_IDS, length=(3, 12))


def fusion_model():
    """Order 3 over about 20 of the 81 ids: the synthetic head is near-flat, so at weight 1 the model decides which ids a beam takes
    and, with a bonus of 0.3 per token, how long it runs."""
    return ngram_ref.train(fusion_corpus(), LM_ORDER, V_MODEL)


def probe_rows(seqs, order, V, start=2):
    """{kind: token rows (index 0 the start token)}: contexts that were seen, wholly unseen ones, ones with an unseen id in the middle
    (the longer contexts do not exist as grams, so no backoff weight is added for them, while the shorter ones do), and ones shorter
    than order - 1 that start at <s>."""
    a = [s for s in seqs if len(s) >= 9][:3]
    unseen = [V - 1 - (i % 3) for i in range(9)]
    rows = {"seen": [[start] + s[:k] for s in a for k in (len(s), max(order - 1, 1), order)],
            "unseen": [[start] + unseen[:k] for k in (1, 2, order - 1 or 1, order, 9)],
            "middle": [[start] + s[:4] + [V - 1] + s[5:5 + k] for s in a for k in (0, 1, 2, 3)] + [[start] + s[:6] + [V - 2, V - 1] for s in a],
            "short": [[start]] + [[start] + s[:k] for s in a for k in range(1, max(order - 1, 2))]}
    return rows
