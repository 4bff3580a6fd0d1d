"""CPU tests of speech_to_text.py: the corpus walk score_many and align_many share (a pure host function), and where the model and
its decoder holders live.  tests/golden/speech_to_text_state_dict_keys.txt is ``sorted(model.state_dict())`` of
``SpeechT5ForSpeechToTextMI355X(layers=1, decoder_layers=2)``, one name per line, recorded at the commit before the model got a module
of its own."""
import importlib
import os

import pytest
import torch

la = importlib.import_module("loco-asr_amd")
dec = importlib.import_module("loco-asr_amd.decoder")
stt = importlib.import_module("loco-asr_amd.speech_to_text")

SIZES = [2, 1, 3]
LENGTHS = [3, 1, 5, 2, 2, 4]


def label_rows():
    return [torch.arange(10 * u + 4, 10 * u + 4 + n) for u, n in enumerate(LENGTHS)]


def walk(pack, sizes=SIZES, rows=None, what="score_many", check_row=lambda lab: lab.to(torch.long)):
    return stt.corpus_packs(what, sizes, pack, label_rows() if rows is None else rows, check_row)


def check_padding(packs, rows):
    for _, us, lab in packs:
        assert lab.dtype == torch.long and lab.shape[0] == us.stop - us.start
        for i, u in enumerate(range(us.start, us.stop)):
            n = len(rows[u])
            assert torch.equal(lab[i, :n], rows[u])
            assert bool((lab[i, n:] == -100).all())


@pytest.mark.parametrize("pack,batches,utterances,shapes", [
    (1, [[0], [1], [2]], [(0, 2), (2, 3), (3, 6)], [(2, 3), (1, 5), (3, 4)]),
    (2, [[0, 1], [2]], [(0, 3), (3, 6)], [(3, 5), (3, 4)]),
    (3, [[0, 1, 2]], [(0, 6)], [(6, 5)]),
    (8, [[0, 1, 2]], [(0, 6)], [(6, 5)]),
])
def test_walk_packs(pack, batches, utterances, shapes):
    packs = walk(pack)
    assert [idx for idx, _, _ in packs] == batches
    assert [(us.start, us.stop) for _, us, _ in packs] == utterances
    assert [tuple(lab.shape) for _, _, lab in packs] == shapes
    check_padding(packs, label_rows())


def test_walk_skips_an_empty_batch():
    rows = label_rows()
    packs = walk(2, sizes=[2, 0, 1, 0, 3, 0])
    assert [idx for idx, _, _ in packs] == [[0, 2], [4]]
    assert [(us.start, us.stop) for _, us, _ in packs] == [(0, 3), (3, 6)]
    assert [tuple(lab.shape) for _, _, lab in packs] == [(3, 5), (3, 4)]
    check_padding(packs, rows)
    assert walk(2, sizes=[0, 0], rows=[]) == []


def test_walk_hands_out_what_check_row_returns():
    packs = walk(3, check_row=lambda lab: (lab + 1).to(torch.long))
    check_padding(packs, [r + 1 for r in label_rows()])


@pytest.mark.parametrize("what", ["score_many", "align_many"])
def test_walk_argument_errors(what):
    with pytest.raises(ValueError, match=f"^{what}: 5 label rows for 6 utterances$"):
        walk(2, rows=label_rows()[:5], what=what)
    with pytest.raises(ValueError, match="^pack must be >= 1$"):  # the one message of the three that never carried the caller's name
        walk(0, what=what)
    rows = label_rows()
    rows[4] = rows[4][None]
    with pytest.raises(ValueError, match=f"^{what}: labels\\[4\\] must be a 1-D tensor of token ids$"):
        walk(2, rows=rows, what=what)
    rows[4] = [7, 2]
    with pytest.raises(ValueError, match=f"^{what}: labels\\[4\\] must be a 1-D tensor of token ids$"):
        walk(2, rows=rows, what=what)
    # the count is looked at before pack, pack before the rows, and a row's shape before the caller's own check of it
    with pytest.raises(ValueError, match="label rows for"):
        walk(0, rows=rows[:5], what=what)
    with pytest.raises(ValueError, match="pack must be"):
        walk(0, rows=rows, what=what)
    seen = []
    with pytest.raises(ValueError, match="labels\\[4\\]"):
        walk(2, rows=rows, what=what, check_row=lambda lab: seen.append(lab) or lab)
    assert len(seen) == 4


def test_module_layout():
    m = la.SpeechT5ForSpeechToTextMI355X(layers=1, decoder_layers=2)
    assert type(m).__module__.endswith("speech_to_text") and type(m) is stt.SpeechT5ForSpeechToTextMI355X
    for holder in (m.speecht5.decoder, m.text_decoder_postnet):
        assert getattr(dec, type(holder).__name__) is type(holder)
        assert type(holder).__qualname__ == type(holder).__name__
    assert m._decoder_runtime.last_lengths is None
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "speech_to_text_state_dict_keys.txt")) as fh:
        want = fh.read().split()
    assert len(want) == 90 and sorted(m.state_dict()) == want


def imported(module):
    """Every module name the file of ``module`` imports, at any depth of nesting: "torch", ".decoder", ".synth.HIDDEN", ..."""
    import ast
    names = set()
    with open(importlib.import_module("loco-asr_amd." + module).__file__) as fh:
        for node in ast.walk(ast.parse(fh.read())):
            if isinstance(node, ast.Import):
                names |= {a.name for a in node.names}
            elif isinstance(node, ast.ImportFrom):
                base = "." * node.level + (node.module or "")
                names |= {base} | {base.rstrip(".") + "." + a.name for a in node.names}
    return names


def test_who_imports_whom():
    halves = {".encoder", ".decoder", ".speech_to_text", ".text_encoder"}
    assert not {n for n in imported("holders") if n.startswith(".")}
    assert not imported("encoder") & (halves - {".encoder"})
    assert not imported("decoder") & (halves - {".decoder"})
    assert {".encoder", ".decoder", ".holders"} <= imported("speech_to_text") and ".text_encoder" not in imported("speech_to_text")
