"""The beam restatement of tests/decoder_beam_ref.py with shallow fusion (include/loco_asr.h, "n-gram language model"): step 1 scores a
candidate ``s = (run[k] + float64(lp[k][v])) + bonus[k][v]``, two additions, each rounded once; steps 2 - 7 are the rule's, restated here
in full so that the fused and the plain restatement can be compared array for array.  ``bonus=None`` is the plain rule.
``search`` drives a group with the acoustic log-probabilities of a function and the bonus of an n-gram model (tests/ngram_ref.py) on the
restatement's own token rows."""
import numpy as np

import decoder_beam_ref as ref
from decoder_beam_ref import EOS, FINISHED, PAD, candidate_key, score_above


def fused_bonus(lm_rows, weight, token_bonus):
    """bonus = weight * lm + token_bonus in float64, a multiplication and an addition, each rounded once."""
    return np.float64(weight) * np.asarray(lm_rows, np.float64) + np.float64(token_bonus)


class FusedBeamGroup(ref.BeamGroup):
    def step(self, lp, bonus=None, dtype=np.float32):
        K, V, S = self.K, self.V, self.S
        lp = np.asarray(lp, dtype=dtype)
        assert lp.shape == (K, V)
        if bonus is not None:
            bonus = np.asarray(bonus, np.float64)
            assert bonus.shape == (K, V)
        if not self.open:
            return False
        t = int(self.pos[0])
        if t < 0 or t + 1 >= S:
            self.parent[:] = np.arange(K)
            self.count[:] = 0
            return False
        cur, cap = t + 1, int(self.caps[0])
        cands = []
        for k in range(K):
            if not self.alive[k]:
                continue
            for v in range(V):
                s = np.float64(self.run[k]) + np.float64(lp[k, v])
                if bonus is not None:
                    s = s + bonus[k, v]
                cands.append((float(s), k * V + v))
        cands.sort(key=lambda c: candidate_key(*c))
        cands = cands[:2 * K]
        at_cap = cur + 1 >= cap or cur + 1 >= S
        hits = [c[1] % V == EOS or at_cap for c in cands]
        m = [(float(self.fin_score[e]), ("old", e)) for e in range(min(max(int(self.fin_n[0]), 0), K))]
        unsat = bool(self.unsat[0])
        den_cur = float(self.den[min(max(cur, 1), len(self.den) - 1)])
        if unsat and not (self.early == 1 and len(m) >= K):
            for c in range(min(K, len(cands))):
                if not hits[c]:
                    continue
                sc = float(np.float64(cands[c][0]) / np.float64(den_cur))
                at = len(m)
                while at > 0 and score_above(sc, m[at - 1][0]):
                    at -= 1
                m.insert(at, (sc, ("new", c)))
        m = m[:K]
        nxt = [c for c in range(len(cands)) if not hits[c]][:K]
        done = True
        if nxt:
            L = min(max(cap - 1 if (self.early == 2 and self.penalty_positive) else cur, 1), len(self.den) - 1)
            worst = m[K - 1][0] if len(m) >= K else -1e9
            with np.errstate(all="ignore"):
                unsat = unsat and bool(np.float64(cands[nxt[0]][0]) / np.float64(self.den[L]) > worst)
            done = (not unsat) or (self.early == 1 and len(m) >= K)
        old = {n: getattr(self, n).copy() for n in ("fin_score", "fin_sum", "fin_len", "fin_tok", "fin_tlp")}
        for q, (sc, (kind, i)) in enumerate(m):
            if kind == "new":
                k, tok = divmod(cands[i][1], V)
                self.fin_tok[q, :cur], self.fin_tok[q, cur] = self.tokens[k, :cur], tok
                self.fin_tlp[q, :cur], self.fin_tlp[q, cur] = self.tlp[k, :cur], lp[k, tok]
                self.fin_score[q], self.fin_sum[q], self.fin_len[q] = sc, cands[i][0], cur + 1
            elif i != q:
                n = min(max(int(old["fin_len"][i]), 0), S)
                self.fin_tok[q, :n], self.fin_tlp[q, :n] = old["fin_tok"][i, :n], old["fin_tlp"][i, :n]
                self.fin_score[q], self.fin_sum[q], self.fin_len[q] = sc, old["fin_sum"][i], old["fin_len"][i]
        cnt = self.cnt.copy()
        for r in range(K):
            par, tok, al, n, l, sc = r, PAD, 0, int(cnt[r]), 0.0, -1e9
            if r < len(nxt):
                par, tok = divmod(cands[nxt[r]][1], V)
                al, l, sc, n = 1, lp[par, tok], cands[nxt[r]][0], int(cnt[par]) + (tok != PAD)
            self.tokens[r, cur], self.tlp[r, cur], self.run[r], self.alive[r] = tok, l, sc, al
            self.parent[r], self.count[r], self.lengths[r] = par, 0 if done else cur, cur + 1
            if done:
                self.status[r] = FINISHED
            else:
                self.pos[r], self.cur[r], self.cnt[r] = t + 1, tok, n
        self.unsat[0], self.fin_n[0] = int(unsat), len(m)
        return True


def lm_rows(ngram_ref, model, group):
    """float64 [K, V]: the n-gram model's next-token log-probabilities on the group's own token rows."""
    cur = int(group.pos[0]) + 1
    return np.stack([ngram_ref.next_logprobs(model, group.tokens[k, :cur]) for k in range(group.K)])


def search(logprob_fn, K, V, cap, ngram_ref=None, model=None, weight=0.0, token_bonus=0.0, length_penalty=1.0, early_stopping=False, S_max=None,
           dtype=np.float32):
    """Run one group to its end; ``logprob_fn(rows)`` maps the running beams' token rows (int [K, cur]) to log-probabilities [K, V];
    ``model`` (an ngram_ref.Model; None: no fusion) gives the bonus."""
    g = FusedBeamGroup(K, V, cap if S_max is None else S_max, cap, length_penalty, early_stopping)
    while g.open:
        cur = int(g.pos[0]) + 1
        bonus = fused_bonus(lm_rows(ngram_ref, model, g), weight, token_bonus) if model is not None else None
        assert g.step(logprob_fn(g.tokens[:, :cur].copy()), bonus, dtype=dtype)
        g.reorder()
    return g
