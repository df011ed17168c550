"""Pin tests/beam_penalty_ref.py - beam search under the checkpoint's repetition penalty - on HF's OWN
`generate(num_beams=k, repetition_penalty=p, do_sample=False)` of a tiny seeded Qwen2 decoder (fp32, CPU; the model of
tests/test_oracle_beam.py).  Qwen2-VL / Qwen2.5-VL instruct checkpoints ship `repetition_penalty` 1.05 in generation_config.json and
HF merges it into every `generate` call the reference makes, beam search included.  In beam search HF applies the processor to the
LOG-SOFTMAX output; the greedy path's order (penalise the raw logits, then log-softmax) gives other answers, and one case here must
show it.  The product's host bookkeeping (`BeamSearcher`) fed penalised log-probabilities with logz = 0 - what generate_beam gives it
from `owc_beam_candidates_penalized` - equals the restatement on a batch."""
import numpy as np
import pytest

from oracle import beam_np as BM
from tests.beam_penalty_ref import beam_search_penalized

V = 97


@pytest.fixture(scope="module")
def tiny_lm():
    import torch
    from transformers import Qwen2Config, Qwen2ForCausalLM

    torch.manual_seed(7)
    cfg = Qwen2Config(vocab_size=V, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4,
                      num_key_value_heads=2, max_position_embeddings=128, tie_word_embeddings=False)
    m = Qwen2ForCausalLM(cfg).eval().float()
    with torch.no_grad():
        for p in m.parameters():          # wider logits than the default init: beams of different quality
            p.mul_(3.0)
    return m


def _hf_beams(m, prompt, k, T, eos, pad, **kw):
    import torch

    with torch.no_grad():
        out = m.generate(input_ids=torch.tensor([prompt]), attention_mask=torch.ones(1, len(prompt), dtype=torch.long), num_beams=k,
                         do_sample=False, max_new_tokens=T, eos_token_id=eos, pad_token_id=pad, use_cache=True, **kw)
    new = out[0, len(prompt):].tolist()
    return np.array(new + [pad] * (T - len(new)))


def _logits_fn(m, prompt):
    import torch

    def fn(conts):
        with torch.no_grad():
            return m(input_ids=torch.tensor([prompt + c for c in conts])).logits[:, -1, :].float().numpy()
    return fn


# (k, p, length_penalty): every k in {2, 3, 4} with every p in {0.8, 1.05, 1.3, 2.0}, plus two length penalties != 1
CASES = [(k, p, 1.0) for k in (2, 3, 4) for p in (0.8, 1.05, 1.3, 2.0)] + [(3, 1.3, 0.5), (2, 2.0, 2.0)]


def test_penalised_beam_search_matches_hf_generate(tiny_lm):
    m, pad, T = tiny_lm, 0, 8
    r = np.random.default_rng(2024)
    changed = raw_missed = eos_met = 0
    for n, (k, p, lp) in enumerate(CASES):
        prompt = r.integers(1, V, 5 + n % 4).tolist()
        fn = _logits_fn(m, prompt)
        # an EOS id the search meets: the most frequent token of an EOS-free penalised run of the restatement
        free, _ = beam_search_penalized(fn, prompt, k, T, -1, pad, repetition_penalty=p, length_penalty=lp)
        vals, counts = np.unique(free, return_counts=True)
        eos = int(vals[np.argsort(-counts, kind="stable")][0])
        want = _hf_beams(m, prompt, k, T, eos, pad, repetition_penalty=p, length_penalty=lp)
        got, _ = beam_search_penalized(fn, prompt, k, T, eos, pad, repetition_penalty=p, length_penalty=lp)
        assert np.array_equal(got, want), (k, p, lp, got, want)
        eos_met += int(eos in want)
        changed += int(not np.array_equal(want, _hf_beams(m, prompt, k, T, eos, pad, length_penalty=lp)))
        raw, _ = beam_search_penalized(fn, prompt, k, T, eos, pad, repetition_penalty=p, length_penalty=lp, raw_form=True)
        raw_missed += int(not np.array_equal(raw, want))
    assert eos_met >= 1, "no case ended a hypothesis at EOS"
    assert changed >= 1, "the penalty changed no answer: the cases would not see a missing penalty"
    assert raw_missed >= 1, "no case separates the log-prob form from the raw-logit form"


@pytest.mark.parametrize("k", [2, 3])
def test_restatement_at_penalty_one_is_beam_np(tiny_lm, k):
    m, pad, T = tiny_lm, 0, 7
    r = np.random.default_rng(11 * k)
    for trial in range(3):
        prompt = r.integers(1, V, 6 + trial).tolist()
        fn = _logits_fn(m, prompt)
        for eos in (int(r.integers(1, V)), -1):
            a, sa = BM.beam_search(fn, len(prompt), k, T, eos, pad)
            b, sb = beam_search_penalized(fn, prompt, k, T, eos, pad, repetition_penalty=1.0)
            assert np.array_equal(a, b) and sa == sb


def test_product_bookkeeping_under_the_penalty_equals_the_restatement():
    """`BeamSearcher` on B prompts at once, fed per running row what `generate_beam` feeds it under a penalty: logz = 0 and the
    2 x num_beams largest PENALISED log-probabilities (seen = prompt + the row's own hypothesis), on a synthetic "model" (logits = a
    seeded function of the sequence), with EOS ids the search meets: same tokens, same scores as the restatement prompt by prompt."""
    from lmms_owc_amd.engine.beam import BeamSearcher
    from oracle.qwen2vl_np import repetition_penalty_scores

    Vs, B, T = 61, 6, 9
    rng = np.random.default_rng(9)
    table = rng.normal(size=(Vs, Vs, Vs)).astype(np.float32) * 2.5
    prompts = [rng.integers(0, Vs, 4 + s).tolist() for s in range(B)]

    def logits_of(s: int, seq: list) -> np.ndarray:
        a = (s * 7 + len(seq)) % Vs
        b = seq[-1] if seq else prompts[s][-1]
        c = seq[-2] if len(seq) > 1 else prompts[s][0]
        return table[a, b] + 0.5 * table[c, a]

    for k, eos, p in ((2, 11, 1.3), (3, 40, 2.0), (4, 7, 0.8)):
        want = [beam_search_penalized(lambda conts, s=s: np.stack([logits_of(s, c) for c in conts]), prompts[s], k, T, eos, 0,
                                      repetition_penalty=p) for s in range(B)]
        bs = BeamSearcher(B, k, T, eos, 0)
        seqs = [[[] for _ in range(k)] for _ in range(B)]
        more = True
        while more:
            lg = np.stack([np.stack([logits_of(s, seqs[s][j]) for j in range(k)]) for s in range(B)])       # [B, k, V]
            lp = BM.log_softmax(lg)
            v = np.stack([np.stack([repetition_penalty_scores(lp[s, j], prompts[s] + seqs[s][j], p) for j in range(k)])
                          for s in range(B)])
            order = np.lexsort((np.broadcast_to(np.arange(Vs), v.shape), -v.astype(np.float64)), axis=-1)[..., : 2 * k]
            parent, token, more = bs.step(np.zeros((B, k), np.float32), np.take_along_axis(v, order, -1), order.astype(np.int32))
            seqs = [[seqs[s][parent[s, j]] + [int(token[s, j])] for j in range(k)] for s in range(B)]
        toks, scores = bs.result()
        for s in range(B):
            assert np.array_equal(toks[s], want[s][0]), (k, eos, p, s, toks[s], want[s][0])
            assert abs(scores[s] - want[s][1]) < 1e-4
