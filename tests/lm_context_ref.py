"""Restatement of ``carry`` mode's plan in numpy, written from the rules and not from ``lm.py``:

* a chunk is one utterance; an utterance longer than ``n_positions - keep`` is cut into pieces of that size (the last piece is the rest);
* the slot holds the stream tokens ``[base, base + P)``; a chunk of L tokens that does not fit (``P + L > n_positions``) first rebases the
  slot onto the last ``keep`` stream tokens before the chunk;
* the chunk is then scored behind the slot and appended to it.
"""
import numpy as np


def chunks(utt_lens, n_positions, keep):
    """(start, end) of every chunk in the recording's token stream."""
    size = n_positions - keep
    bounds = np.concatenate([[0], np.cumsum(np.asarray(utt_lens, np.int64))])
    out = []
    for a, b in zip(bounds[:-1], bounds[1:]):
        cuts = np.arange(a, b, size)
        out += [(int(c), int(min(c + size, b))) for c in cuts]
    return out


def carry_plan(utt_lens, n_positions, keep):
    """[(base, P, chunk_start, chunk_end, rebased)] -- the slot's state is re-derived per chunk from where its contents begin."""
    assert 1 <= keep < n_positions
    plan, base = [], 0
    for start, end in chunks(utt_lens, n_positions, keep):
        rebased = end - base > n_positions  # tokens [base, end) would not fit the slot
        if rebased:
            base = start - keep
        plan.append((base, start - base, start, end, bool(rebased)))
    return plan


def left_context(plan):
    """Left context of every scored token (all but the recording's first), by stream position."""
    ctx = {}
    for base, P, a, b, _ in plan:
        for p in range(a, b):
            assert p not in ctx
            ctx[p] = p - base
    return ctx
