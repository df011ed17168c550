"""Beam search under HF's repetition penalty, restated for the tests (`oracle/beam_np.beam_search` + the processor).

HF's `_beam_search` runs its logits processors on the LOG-SOFTMAX output (`log_probs = logits_processor(input_ids,
log_softmax(logits.float()))`), unlike its greedy / sampled loops, which process the raw logits.  With `repetition_penalty` p every
id in a hypothesis's input_ids - the prompt, image placeholders included, and the hypothesis's own generated tokens - gets
lp < 0 ? lp * p : lp / p, once per distinct id.  `raw_form=True` restates the OTHER order (penalise the raw logits, then
log-softmax), which is NOT what HF does: the tests keep it to show that the two differ.  At p = 1 the result equals
`beam_np.beam_search` exactly (the same arithmetic, the processor skipped).  Pinned on HF's own `generate` in
tests/test_oracle_beam_penalty.py."""

from __future__ import annotations

import numpy as np

from oracle import beam_np as BM
from oracle.qwen2vl_np import repetition_penalty_scores

NEG = BM.NEG


def beam_search_penalized(logits_fn, prompt_ids, num_beams: int, max_new_tokens: int, eos_token_id: int, pad_token_id: int,
                          repetition_penalty: float = 1.0, length_penalty: float = 1.0, early_stopping=False,
                          raw_form: bool = False) -> tuple[np.ndarray, float]:
    """One prompt (`prompt_ids`: its token ids).  `logits_fn(list of num_beams generated-token lists) -> float32 [num_beams, vocab]` =
    the next-token logits of prompt + each continuation.  Returns (generated tokens of the best hypothesis padded to max_new_tokens,
    its score)."""
    prompt = [int(t) for t in prompt_ids]
    p = float(repetition_penalty)

    def scores(running):
        lg = np.asarray(logits_fn(running), np.float32)
        if p == 1.0:
            return BM.log_softmax(lg)
        if raw_form:
            return BM.log_softmax(np.stack([repetition_penalty_scores(lg[j], prompt + running[j], p) for j in range(len(running))]))
        lp = BM.log_softmax(lg)
        return np.stack([repetition_penalty_scores(lp[j], prompt + running[j], p) for j in range(len(running))])

    k = num_beams
    running = [[] for _ in range(k)]
    run_scores = np.full(k, NEG, np.float32)
    run_scores[0] = 0.0
    fin = [[] for _ in range(k)]
    fin_scores = np.full(k, NEG, np.float32)
    is_fin = np.zeros(k, bool)
    unsat = True
    g = 0
    while True:   # the loop of beam_np.beam_search, fed the processed log-probs
        logp = scores(running) + run_scores[:, None]
        V = logp.shape[1]
        top = BM.topk_desc(logp.reshape(-1), 2 * k)
        c_scores = logp.reshape(-1)[top].astype(np.float32)
        c_seqs = [running[i // V] + [int(i % V)] for i in top]
        hits = np.array([s[-1] == eos_token_id or g + 1 >= max_new_tokens for s in c_seqs])
        r_scores = (c_scores + hits.astype(np.float32) * np.float32(NEG)).astype(np.float32)
        nxt = BM.topk_desc(r_scores, k)
        did = hits & (np.arange(2 * k) < k)
        f = (c_scores / np.float32((g + 1) ** length_penalty)).astype(np.float32)
        if bool(is_fin.all()) and early_stopping is True:
            f = f + np.float32(NEG)
        if not unsat:
            f = f + np.float32(NEG)
        f = f + (~did).astype(np.float32) * np.float32(NEG)
        m_scores = np.concatenate([fin_scores, f])
        m_seqs = fin + c_seqs
        m_fin = np.concatenate([is_fin, did])
        keep = BM.topk_desc(m_scores, k)
        fin, fin_scores, is_fin = [m_seqs[i] for i in keep], m_scores[keep].astype(np.float32), m_fin[keep]
        running, run_scores = [c_seqs[i] for i in nxt], r_scores[nxt]
        g += 1
        hyp_len = max_new_tokens if (early_stopping == "never" and length_penalty > 0.0) else g
        best_possible = run_scores[0] / np.float32(hyp_len ** length_penalty)
        worst_fin = np.where(is_fin, fin_scores.min(), np.float32(NEG))
        unsat = unsat and bool((best_possible > worst_fin).any())
        open_beam = not (bool(is_fin.all()) and early_stopping is True)
        if not (unsat and open_beam and not bool(hits.all())):
            break
    out = np.full(max_new_tokens, pad_token_id, np.int64)
    out[: len(fin[0])] = fin[0]
    return out, float(fin_scores[0])
