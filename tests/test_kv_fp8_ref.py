"""CPU checks of the fp8 KV cache's numpy restatement (tests/kv_fp8_ref.py) and of the host-side switches."""
import ctypes as C

import numpy as np
import pytest

from oracle import qwen2vl_np as Q
from tests import kv_fp8_ref as R
from tests import recipes


@pytest.fixture(scope="module")
def model():
    cfg = recipes.tiny_cfg()
    return cfg, recipes.qwen2vl_weights(cfg, 1234)


def test_reference_loop_with_a_plain_cache_is_q_generate(model):
    cfg, w = model
    ids = np.random.default_rng(3).integers(1, 490, 13).astype(np.int64)
    forced = np.random.default_rng(4).integers(1, 490, 5)
    toks, logits = R.generate_forced(w, cfg, ids, 5, forced)
    o_toks, o_logits = Q.generate(w, cfg, ids, None, [], 5, bf16=True, return_logits=True, forced_tokens=forced)
    assert np.array_equal(logits, o_logits) and np.array_equal(toks, o_toks)


def test_quantising_cache_leaves_the_first_step_alone_and_moves_the_rest(model):
    cfg, w = model
    ids = np.random.default_rng(5).integers(1, 490, 12).astype(np.int64)
    forced = np.random.default_rng(6).integers(1, 490, 4)
    _, plain = R.generate_forced(w, cfg, ids, 4, forced)
    cache = R.Fp8KVCache(cfg.text.num_hidden_layers)
    _, quant = R.generate_forced(w, cfg, ids, 4, forced, cache=cache)
    assert np.array_equal(quant[0], plain[0])            # prefill attention reads bf16
    assert not np.array_equal(quant[1:], plain[1:])      # decode steps read the quantised rows
    assert np.abs(quant - plain).max() <= 0.15 * np.abs(plain).max()
    k = cache.k[0]                                       # stored rows are code * scale: quantising them again changes nothing
    assert k.shape[1] == len(ids) + 3 and np.array_equal(R.quant_dequant_rows(k), k)


def test_kv_dtype_is_validated():
    from lmms_owc_amd.engine.llava import LlavaDims
    from lmms_owc_amd.engine.qwen2vl import Qwen2VLDims, kv_bytes_per_token

    with pytest.raises(ValueError, match="kv_dtype"):
        Qwen2VLDims(kv_dtype="int4")
    with pytest.raises(ValueError, match="kv_dtype"):
        LlavaDims(kv_dtype="fp4")
    with pytest.raises(ValueError, match="head_dim 128"):
        Qwen2VLDims(kv_dtype="fp8", n_q_heads=68, n_kv_heads=4)     # 17 query heads per kv head: not the fused kernel's shape
    assert Qwen2VLDims().kv_dtype == "bf16" and LlavaDims(kv_dtype="fp8").kv_dtype == "fp8"
    d16, d8 = Qwen2VLDims(), Qwen2VLDims(kv_dtype="fp8")
    assert kv_bytes_per_token(d16) == 28 * 2 * 4 * 128 * 2
    assert kv_bytes_per_token(d8) <= 0.56 * kv_bytes_per_token(d16)   # (128 + 4) / 256 + 1 / n_layers


def test_kvcache_struct_defaults_to_bf16():
    from lmms_owc_amd import _lib

    c = _lib.KvCache(1, 2, 3, 4)
    assert (c.dtype, c.n_slots, c.s_max) == (_lib.KV_BF16, 3, 4) and c.dtype == 0
    assert c.k_scale is None and c.v_scale is None and c.k_stage is None and c.v_stage is None
    # appended fields: the bf16 prefix keeps its offsets
    assert _lib.KvCache.k.offset == 0 and _lib.KvCache.n_slots.offset == 2 * C.sizeof(C.c_void_p)
    assert _lib.KvCache.dtype.offset == _lib.KvCache.s_max.offset + 4
    assert _lib.ABI_VERSION >= 21


def test_beam_requests_are_refused_on_an_fp8_cache():
    from lmms_owc_amd.engine.qwen2vl import Qwen2VLDims
    from lmms_owc_amd.models._base import beams_from_gen_kwargs

    assert beams_from_gen_kwargs({"num_beams": 2}, Qwen2VLDims()) == 2
    assert beams_from_gen_kwargs({"num_beams": 1}, Qwen2VLDims(kv_dtype="fp8")) == 1
    with pytest.raises(ValueError, match="kv_dtype=fp8"):
        beams_from_gen_kwargs({"num_beams": 2}, Qwen2VLDims(kv_dtype="fp8"))
