"""Host-side inputs shared by the tests of sampled decoding under the repetition penalty (tests/test_logits_consumers_gpu.py on the
GPU, tests/test_oracle_sampling.py on the CPU): numpy only."""
import numpy as np

from oracle import np_ops


def host_bitmap(hists, V, spare_words=3):
    """Seen-token bitmap built on the HOST (owc_seen_mark drops ids >= V): one row per history, `spare_words` more words per row than
    the vocabulary needs.  Every bit the kernels must IGNORE is set: the bits at and above V of a ragged last word, all spare words."""
    words = (V + 31) // 32
    bits = np.zeros((len(hists), words + spare_words), np.uint32)
    for s, h in enumerate(hists):
        h = np.unique(np.asarray(h, np.int64))
        np.bitwise_or.at(bits[s], h >> 5, np.uint32(1) << (h & 31).astype(np.uint32))
    if V % 32:
        bits[:, words - 1] |= np.uint32((0xFFFFFFFF << (V % 32)) & 0xFFFFFFFF)
    bits[:, words:] = np.uint32(0xFFFFFFFF)
    return bits


CONFIGS = [(0.8, 0, None), (0.7, 40, 0.8), (1.5, 7, 0.6)]


def sampling_row(V):
    """One row and one history (penalty 1.3) on which the penalty MATTERS for every config of CONFIGS: half of the 16 largest logits
    are in the history (plus 200 random ids), so the oracle's kept set moves.  The CPU tests bound the write-back's cost on the same rows."""
    r = np.random.default_rng(V)
    row = np_ops.bf16_round((r.standard_normal(V) * 2.5).astype(np.float32))
    top = np.argsort(-row, kind="stable")[:16]
    hist = np.unique(np.concatenate([top[::2], r.integers(0, V, 200)]))
    return row, hist, 1.3


def shipped_config_rows(V, seed=12):
    """256 rows of integer-valued logits: a background of round(2 N(0, 1)) and, per row, 8 top tokens with integer values in 16 .. 24
    (many tied maxima), 4 of them in the row's history.  At 1.05 a seen 20 becomes 19.0476 and rounds to bf16 19.0 (the bf16 step
    between 16 and 32 is 0.125): it ties with an unseen 19 it beats in fp32.  (The seed: one of those at which numpy
    finds such rows at both vocabularies - 8 of 256 at 152 064, 3 at 520.)"""
    r = np.random.default_rng(seed)
    x = np.round(r.standard_normal((256, V)) * 2).astype(np.float32)
    hists = []
    for i in range(256):
        top = r.choice(V, 8, replace=False)
        x[i, top] = r.integers(16, 25, 8)
        hists.append(np.concatenate([top[:4], r.integers(0, V, 30)]))
    return x, hists
