"""The fp8 (e4m3fn) KV cache, restated for the tests on top of oracle/qwen2vl_np.py and oracle/fp8_np.py.

`kv_dtype="fp8"` stores every (token, kv head) row of K (after RoPE) and V as `fp8_np.quantize_rows` codes + one fp32 scale.  Prefill
attention reads the rows it has just computed in bf16 (so the first-token logits equal the bf16 cache's bit for bit); a decode step
attends dequantised rows only, its own new row included.  `Fp8KVCache.update` is exactly that: it stores
`e4m3_decode(codes) * scale`, hands a multi-token call (the prefill) its unquantised k / v back and a one-token call (a decode
step) the stored rows.  `generate_forced` is the teacher-forced greedy loop of `Q.generate` with the cache as a parameter.
"""

from __future__ import annotations

import numpy as np

from oracle import fp8_np as F
from oracle import qwen2vl_np as Q
from oracle.np_ops import maybe_bf16


def quant_dequant_rows(x: np.ndarray) -> np.ndarray:
    """[..., head_dim] -> the values an fp8 cache returns for these rows (float32)."""
    flat = np.asarray(x, np.float32).reshape(-1, x.shape[-1])
    codes, scale = F.quantize_rows(flat)
    return (F.e4m3_decode(codes) * scale[:, None]).astype(np.float32).reshape(x.shape)


class Fp8KVCache(Q.KVCache):
    def update(self, i, k, v):
        kq, vq = quant_dequant_rows(k), quant_dequant_rows(v)
        first = self.k[i] is None
        self.k[i] = kq if first else np.concatenate([self.k[i], kq], 1)
        self.v[i] = vq if first else np.concatenate([self.v[i], vq], 1)
        if k.shape[1] > 1:          # prefill: attention over the rows of this call, unquantised
            assert first, "an fp8-cache prefill attends only the keys it writes itself"
            return k, v
        return self.k[i], self.v[i]


def generate_forced(w: dict, cfg, input_ids, n_steps: int, forced_tokens=None, *, cache=None, bf16=True):
    """Text-only prompt -> (argmax tokens [n_steps], logits [n_steps, vocab]); the token fed after step j is forced_tokens[j]
    (the step's own argmax when None).  `cache`: a Q.KVCache (default) or an Fp8KVCache."""
    ids = np.asarray(input_ids).astype(np.int64)
    cache = Q.KVCache(cfg.text.num_hidden_layers) if cache is None else cache
    emb = w[Q.T + "embed_tokens.weight"]
    h = Q.llm_forward(w, cfg, maybe_bf16(emb[ids], bf16), np.tile(np.arange(len(ids))[None], (3, 1)), cache, bf16=bf16)
    toks, logits = [], []
    for step in range(n_steps):
        lg = Q.lm_head(w, cfg, h[-1:], bf16=bf16)[0]
        logits.append(lg.copy())
        toks.append(int(Q.greedy_argmax(lg)))
        if step == n_steps - 1:
            break
        feed = toks[-1] if forced_tokens is None else int(forced_tokens[step])
        h = Q.llm_forward(w, cfg, maybe_bf16(emb[np.array([feed])], bf16), np.full((3, 1), len(ids) + step, np.int64), cache, bf16=bf16)
    return np.array(toks), np.stack(logits)
