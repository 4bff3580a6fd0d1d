"""numpy restatement of the beam-search rule of csrc/decoder_beam.hip (include/loco_asr.h states it): HF's ``_beam_search`` with flags
in place of its -1e9 sentinels, scores in float64 and a total order on candidates.  ``BeamGroup`` keeps exactly the arrays the device
keeps for one group, written the way the select kernel writes them, so a test can compare every array after every step;
``reorder`` is the gather the reorder kernels apply afterwards; ``search`` drives a group with a function that maps the running beams'
token rows to log-probabilities."""
import math

import numpy as np

EOS, PAD, START = 2, 1, 2
FREE, OPEN, FINISHED = 0, 1, 2
EARLY = {False: 0, True: 1, "never": 2}


def den_table(length_penalty, n):
    """den[i] = i ** length_penalty in float64, den[0] = 1 (loco_beam_den_table)."""
    return np.array([1.0] + [float(i) ** float(length_penalty) for i in range(1, n)], dtype=np.float64)


def candidate_key(s, index):
    """Sort key of the rule's order: larger score first, lower flat index on a tie; a NaN after every number, NaNs by index."""
    return (1, 0.0, index) if math.isnan(s) else (0, -s, index)


def score_above(a, b):
    """a ranks strictly above b in a finished list: a number above every NaN, NaNs equal."""
    return not math.isnan(a) and (math.isnan(b) or a > b)


class BeamGroup:
    def __init__(self, K, V, S_max, cap, length_penalty=1.0, early_stopping=False, den=None):
        self.K, self.V, self.S, self.cap = int(K), int(V), int(S_max), int(cap)
        self.early = int(EARLY.get(early_stopping, early_stopping))  # False / True / "never", or the config's 0 / 1 / 2
        self.penalty_positive = float(length_penalty) > 0
        self.den = den_table(length_penalty, self.S) if den is None else np.asarray(den, dtype=np.float64)
        K, S = self.K, self.S
        self.status = np.full(K, OPEN, np.int32)
        self.pos = np.zeros(K, np.int32)
        self.caps = np.full(K, self.cap, np.int32)
        self.cur = np.full(K, START, np.int32)
        self.cnt = np.ones(K, np.int32)
        self.lengths = np.ones(K, np.int32)
        self.tokens = np.zeros((K, S), np.int32)
        self.tokens[:, 0] = START
        self.tlp = np.zeros((K, S), np.float32)
        self.run = np.full(K, -1e9, np.float64)
        self.run[0] = 0.0
        self.alive = np.zeros(K, np.int32)
        self.alive[0] = 1
        self.unsat = np.ones(1, np.int32)
        self.fin_n = np.zeros(1, np.int32)
        self.fin_score = np.zeros(K, np.float64)
        self.fin_sum = np.zeros(K, np.float64)
        self.fin_len = np.zeros(K, np.int32)
        self.fin_tok = np.zeros((K, S), np.int32)
        self.fin_tlp = np.zeros((K, S), np.float32)
        self.parent = np.arange(K, dtype=np.int32)  # within the group; the device adds the group's first slot
        self.count = np.zeros(K, np.int32)

    ARRAYS = ("status", "pos", "caps", "cur", "cnt", "lengths", "tokens", "tlp", "run", "alive", "unsat", "fin_n", "fin_score", "fin_sum", "fin_len",
              "fin_tok", "fin_tlp", "parent", "count")

    @property
    def open(self):
        return int(self.status[0]) == OPEN

    def step64(self, lp):
        """``step`` on float64 log-probabilities (a float64 model: what HF computes in double); the history keeps them as float32."""
        return self.step(lp, np.float64)

    def step(self, lp, dtype=np.float32):
        """One step on log-probabilities ``lp`` float32 [K, V].  False: the group took no part (not open, or no room)."""
        K, V, S = self.K, self.V, self.S
        lp = np.asarray(lp, dtype=dtype)
        assert lp.shape == (K, V)
        if not self.open:
            return False
        t = int(self.pos[0])
        if t < 0 or t + 1 >= S:
            self.parent[:] = np.arange(K)
            self.count[:] = 0
            return False
        cur, cap = t + 1, int(self.caps[0])
        cands = [(float(np.float64(self.run[k]) + np.float64(lp[k, v])), k * V + v) for k in range(K) if self.alive[k] for v in range(V)]
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
        # the list: every row written once, from the state before the step
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

    def reorder(self):
        """What the reorder kernels do to the token and log-probability rows after a step: rows 0 .. count - 1 from the parent."""
        if not self.open:
            return
        tok, tlp = self.tokens.copy(), self.tlp.copy()
        for r in range(self.K):
            n, par = int(self.count[r]), int(self.parent[r])
            if par != r:
                self.tokens[r, :n], self.tlp[r, :n] = tok[par, :n], tlp[par, :n]

    def finished(self, n=None):
        """[(tokens list, score, sum of log-probabilities, token log-probabilities f32 [len])] of the list's first n entries."""
        out = []
        for e in range(min(int(self.fin_n[0]), self.K if n is None else n)):
            L = int(self.fin_len[e])
            out.append((self.fin_tok[e, :L].tolist(), float(self.fin_score[e]), float(self.fin_sum[e]), self.fin_tlp[e, :L].copy()))
        return out


def search(logprob_fn, K, V, cap, length_penalty=1.0, early_stopping=False, S_max=None):
    """Run one group to its end: ``logprob_fn(rows)`` maps the running beams' token rows (int [K, cur]) to float32 [K, V]."""
    g = BeamGroup(K, V, cap if S_max is None else S_max, cap, length_penalty, early_stopping)
    while g.open:
        cur = int(g.pos[0]) + 1
        assert g.step(logprob_fn(g.tokens[:, :cur].copy()))
        g.reorder()
    return g


def beam_weights(synth, beta, layers=2, seed=13):
    """Decoder weights whose rows end at different steps: ``synth.decoder_state_dict(seed, layers)`` with an untied
    ``lm_head = 0.05 * embed`` and ``beta * b / (b . b)`` added to its </s> row, ``b`` the last layer's ``final_layer_norm.bias`` --
    close to a constant ``beta`` on the </s> logit."""
    sd = dict(synth.decoder_state_dict(seed, layers=layers))
    head = (0.05 * sd["decoder.prenet.embed_tokens.weight"]).astype(np.float32)
    b = sd[f"decoder.wrapped_decoder.layers.{layers - 1}.final_layer_norm.bias"].astype(np.float64)
    head[EOS] += (beta * b / float(b @ b)).astype(np.float32)
    sd["text_decoder_postnet.lm_head.weight"] = head
    return sd
