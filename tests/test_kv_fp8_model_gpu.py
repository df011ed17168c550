"""Model level of the fp8 (e4m3fn) KV cache (`kv_dtype="fp8"`), tiny Qwen2-VL config of tests/test_fp8_model_gpu.py.

* prefill attention reads bf16 staging: the first-step logits equal the bf16-cache engine's bit for bit;
* every decode step against tests/kv_fp8_ref.py (the numpy model with the quantising cache) under teacher forcing, with the
  project's fp8-model bounds as they are (max 10 %, mean 2 % of max |logit|; token equality where the reference's top-2 margin
  exceeds twice the bound);
* fp8 cache against bf16 cache on the same weights with the caps of test_fp8_vs_bf16_agreement (15 % / 3 % / 75 %);
* the generated tokens do not depend on row compaction, graph replay, the batch, the pruned last prefill layer or the pass
  a sequence finishes in.
"""
import numpy as np
import pytest
import torch

from tests import kv_fp8_ref as R
from tests import recipes
from tests.util import check_forced_steps, to_np

pytestmark = pytest.mark.gpu
KW = dict(v_depth=2, v_embed=160, v_heads=2, v_mlp=640, n_layers=2, d_model=256, n_q_heads=2, n_kv_heads=1, d_ff=512, vocab=512,
          tie_embeddings=False, image_token_id=500, max_positions=512, max_grid=64)


@pytest.fixture(scope="module")
def setup(gpu):
    from lmms_owc_amd.engine.qwen2vl import Qwen2VLDims, Qwen2VLEngine, Qwen2VLWeights

    cfg = recipes.tiny_cfg()
    w = recipes.qwen2vl_weights(cfg, 1234)
    eng = lambda **kw: Qwen2VLEngine(Qwen2VLWeights.from_state_dict(Qwen2VLDims(**KW, **kw), w, gpu))
    return cfg, w, eng(kv_dtype="fp8"), eng(), eng


def _prompts(n, seed=0):
    r = np.random.default_rng(seed)
    return [r.integers(1, 490, 12 + (i % 7)).astype(np.int64) for i in range(n)]   # the first 32: test_fp8_vs_bf16_agreement's


def test_first_step_logits_equal_the_bf16_cache(setup, gpu):
    cfg, w, e8, e16, _ = setup
    assert e8.share_prefix and e16.share_prefix
    r = np.random.default_rng(2)
    head = r.integers(1, 490, 9)                      # a common leading text: the shared-prefix prefill path
    prompts = [np.concatenate([head, r.integers(1, 490, 3 + i)]).astype(np.int64) for i in range(6)]
    t8, l8 = e8.generate(prompts, None, [[] for _ in prompts], 3, return_logits=True)
    t16, l16 = e16.generate(prompts, None, [[] for _ in prompts], 3, return_logits=True)
    assert torch.equal(l8, l16) and torch.equal(t8[:, 0], t16[:, 0])
    grid = [(1, 4, 4)]
    pix = torch.from_numpy(recipes.pixel_values(grid, 7)).to(torch.bfloat16).to(gpu)
    ids = recipes.prompt_ids(cfg, grid, seed=3)
    _, i8 = e8.generate([ids, ids[:-2]], torch.cat([e8.encode_images(pix, grid)] * 2), [grid, grid], 3, return_logits=True)
    _, i16 = e16.generate([ids, ids[:-2]], torch.cat([e16.encode_images(pix, grid)] * 2), [grid, grid], 3, return_logits=True)
    assert torch.equal(i8, i16)


def test_every_step_matches_the_quantising_reference(setup, gpu):
    """128 prompts (the 32 of test_fp8_vs_bf16_agreement first) x 8 teacher-forced steps against tests/kv_fp8_ref.  The reference alone
    has 19 steps with a top-2 margin above twice the logit bound among the first 32 prompts and 103 among the 128 (a property of
    the random-weight miniature, counted with the numpy model): at least 48 token comparisons must really have happened."""
    cfg, w, e8, _, _ = setup
    prompts = _prompts(128)
    ref = [R.generate_forced(w, cfg, p, 8, cache=R.Fp8KVCache(cfg.text.num_hidden_layers)) for p in prompts]
    forced = np.stack([t for t, _ in ref])            # the reference's own continuation
    toks, logits = e8.generate(prompts, None, [[] for _ in prompts], 8, forced_tokens=forced, return_step_logits=True)
    toks, logits = to_np(toks).astype(int), to_np(logits)
    decisive = sum(check_forced_steps(logits[:, b], toks[b], ref[b][1], ref[b][0], 0.10, f"kv-fp8 prompt {b}", mean_frac=0.02)
                   for b in range(len(prompts)))
    print(f"[kv-fp8] {decisive} decisive token steps of {8 * len(prompts)}")
    assert decisive >= 48, decisive


def test_fp8_cache_against_bf16_cache(setup, gpu):
    cfg, w, e8, e16, _ = setup
    prompts = _prompts(32)
    none = [[] for _ in prompts]
    forced = to_np(e16.generate(prompts, None, none, 8)).astype(np.int64)
    t16, l16 = e16.generate(prompts, None, none, 8, forced_tokens=forced, return_step_logits=True)
    t8, l8 = e8.generate(prompts, None, none, 8, forced_tokens=forced, return_step_logits=True)
    assert torch.equal(l8[0], l16[0])
    l8, l16 = to_np(l8)[1:], to_np(l16)[1:]           # the 7 decode steps: [7, 32, vocab]
    scale = np.abs(l16).max(-1)
    mx = (np.abs(l8 - l16).max(-1) / scale).max()
    mean = (np.abs(l8 - l16).mean(-1) / scale).mean()
    agree = (to_np(t8)[:, 1:] == to_np(t16)[:, 1:]).mean()
    print(f"[kv-fp8] fp8 cache vs bf16 cache, 32 prompts x 7 decode steps: max {mx:.4f}, mean {mean:.4f} of max|logit|, top-1 agreement {agree:.3f}")
    assert mx <= 0.15 and mean <= 0.03 and agree >= 0.75, (mx, mean, agree)


def test_tokens_do_not_depend_on_compaction_graph_batch_or_pruning(setup, gpu):
    from lmms_owc_amd import _lib
    from lmms_owc_amd.engine.qwen2vl import Qwen2VLEngine

    cfg, w, e8, _, _ = setup
    prompts = _prompts(40, seed=7)
    none = [[] for _ in prompts]
    free = to_np(e8.generate(prompts, None, none, 20))
    vals, counts = np.unique(free[:, 2:], return_counts=True)
    eos = int(vals[np.argmax(counts)])                # ends many sequences early: rows really leave the batch
    st = {}
    a = e8.generate(prompts, None, none, 20, eos_token_id=eos, compact_rows=True, stats=st)
    b = e8.generate(prompts, None, none, 20, eos_token_id=eos, compact_rows=False)
    assert torch.equal(a, b) and min(st["live_rows_per_step"]) < len(prompts)
    # graph replay of the decode steps against eager launches
    small = prompts[:6]
    eager = Qwen2VLEngine(e8.w, graph_decode=False).generate(small, None, none[:6], 10)
    graph = Qwen2VLEngine(e8.w, graph_decode=True).generate(small, None, none[:6], 10)
    assert torch.equal(eager, graph) and np.array_equal(to_np(eager), free[:6, :10])
    # a prompt alone against the same prompt inside the batch
    for i in (0, 17, 39):
        assert np.array_equal(to_np(e8.generate([prompts[i]], None, [[]], 20))[0], free[i]), i
    # the pruned last prefill layer (fp8 twin of test_fp8_pruned_last_prefill_layer_is_bit_identical)
    lib = _lib.load()
    try:
        assert lib.owc_tuning_set(b"prefill_prune_last", 0) == 0
        p0, l0 = e8.generate(prompts[:5], None, none[:5], 4, return_logits=True)
        assert lib.owc_tuning_set(b"prefill_prune_last", 1) == 0
        p1, l1 = e8.generate(prompts[:5], None, none[:5], 4, return_logits=True)
        assert torch.equal(l0, l1) and torch.equal(p0, p1)
    finally:
        lib.owc_tuning_set(b"prefill_prune_last", 1)


def test_a_carried_sequence_equals_the_one_finished_in_one_pass(setup, gpu):
    """Straggler hand-over under fp8: codes AND scales of the unfinished sequences move into the next pass's cache."""
    cfg, w, e8, _, _ = setup
    passes = [_prompts(40, seed=21), _prompts(20, seed=22)]
    free = to_np(e8.generate(passes[0], None, [[] for _ in passes[0]], 24))
    vals, counts = np.unique(free[:, 2:20], return_counts=True)
    eos = int(vals[np.argmax(counts)])
    ref = [to_np(e8.generate(p, None, [[] for _ in p], 24, eos_token_id=eos, pad_token_id=0)) for p in passes]
    got, state, handed = {}, None, 0
    for k, p in enumerate(passes):
        # (the most frequent token ends about 8 of the 40 sequences inside the cap: the first pass hands over once 3 have ended)
        c = {"in": state, "below": 37 if k == 0 else 0, "tags": [(k, i) for i in range(len(p))]}
        out = to_np(e8.generate(p, None, [[] for _ in p], 24, eos_token_id=eos, pad_token_id=0, carry=c))
        got.update({(k, i): out[i] for i in range(len(p)) if i not in c["unfinished_rows"]})
        got.update(dict(c["finished"]))
        state = c["out"]
        if state is not None:
            handed += len(state["tags"])
            assert len(state["kv_scales"]) == 2 and state["k"].dtype == torch.uint8
    assert state is None and handed >= 3, handed
    for k, p in enumerate(passes):
        for i in range(len(p)):
            assert np.array_equal(got[(k, i)], ref[k][i]), (k, i)


def test_combinations_and_accounting(setup, gpu):
    from lmms_owc_amd import _lib
    from lmms_owc_amd.engine.llava import DIMS, LlavaDims, LlavaEngine, LlavaWeights

    cfg, w, e8, e16, eng = setup
    prompts = _prompts(8, seed=5)
    none = [[] for _ in prompts]
    # fp8 decoder + fp8 cache: generates; first-step logits are those of the fp8 decoder alone
    t_a, l_a = eng(decoder_dtype="fp8", kv_dtype="fp8").generate(prompts, None, none, 6, return_logits=True)
    t_b, l_b = eng(decoder_dtype="fp8").generate(prompts, None, none, 6, return_logits=True)
    assert torch.equal(l_a, l_b) and t_a.shape == (8, 6) and int(t_a.min()) >= 0 and int(t_a.max()) < 512
    # repetition penalty on an fp8 cache
    rp = e8.generate(prompts, None, none, 6, repetition_penalty=1.05)
    assert rp.shape == (8, 6) and np.array_equal(to_np(e8.generate([prompts[3]], None, [[]], 6, repetition_penalty=1.05))[0], to_np(rp)[3])
    # the generic decode path cannot read an fp8 cache: an error, not another result
    lib = _lib.load()
    try:
        assert lib.owc_tuning_set(b"decode_fuse", 0) == 0
        with pytest.raises(_lib.OwcError, match="fp8 KV cache"):
            e8.generate(prompts, None, none, 3)
    finally:
        lib.owc_tuning_set(b"decode_fuse", 1)
    # beam search is refused by the engine as well
    with pytest.raises(ValueError, match="fp8 KV cache"):
        e8.generate_beam(prompts[:2], None, none[:2], 4, 2, eos_token_id=-1)
    # LLaVA engine
    lw = recipes.llava_weights(recipes.tiny_llava_cfg(), 1234)
    le = LlavaEngine(LlavaWeights.from_state_dict(LlavaDims(**{**DIMS["tiny"].__dict__, "kv_dtype": "fp8"}), lw, gpu))
    r = np.random.default_rng(1)
    lp = [r.integers(1, 400, 9 + i) for i in range(3)]
    lt = to_np(le.generate_from_features(lp, None, [np.zeros(0, np.int64)] * 3, 5))
    assert lt.shape == (3, 5) and np.array_equal(to_np(le.generate_from_features([lp[1]], None, [np.zeros(0, np.int64)], 5))[0], lt[1])
    # accounting: codes + scales + the one-layer staging pair against the bf16 cache, same slots and rows: 132 / 256 + 1 / n_layers.
    # The two-layer miniature cannot show the saving (the staging pair is half a bf16 cache there); the same miniature at the 7B
    # model's 28 layers does, and its 28 prefill layers share the staging pair
    assert e16.kv_bytes(64, 400) == 2 * 2 * 1 * 128 * 2 * 64 * 400
    assert e8.kv_bytes(64, 400) == (2 * 2 * 132 + 2 * 128 * 2) * 64 * 400
    from lmms_owc_amd.engine.qwen2vl import Qwen2VLDims, Qwen2VLEngine, Qwen2VLWeights

    deep = {**KW, "n_layers": 28}
    d8, d16 = (Qwen2VLEngine(Qwen2VLWeights.random(Qwen2VLDims(**deep, **kw), gpu, seed=3)) for kw in (dict(kv_dtype="fp8"), {}))
    assert d8.kv_bytes(64, 400) <= 0.56 * d16.kv_bytes(64, 400)
    t8, l8 = d8.generate(prompts, None, none, 4, return_logits=True)
    t16, l16 = d16.generate(prompts, None, none, 4, return_logits=True)
    assert torch.equal(l8, l16)
    held = lambda e: 2 * e._kv[0].numel() * e._kv[0].element_size() + sum(t.numel() * t.element_size() for t in e._kv_aux or ())
    assert held(d8) <= 0.56 * held(d16)     # what the two engines really allocated for the same pass
    e8.generate(prompts, None, none, 3)
    assert e8._kv[0].dtype == torch.uint8 and e8.held_bytes() > 0
    e8.release_kv()
    assert e8._kv is None and e8._kv_aux is None


@pytest.mark.parametrize("model_type,name", [("qwen2-vl", "tiny"), ("qwen2-vl", "tiny25"), ("llava", "tiny-next")])
def test_kv_dtype_through_the_plugin(gpu, model_type, name):
    """`--model_args kv_dtype=fp8` on the plug-ins: strings come back, batch-invariant; an unknown dtype and a beam-search request are
    refused - the latter while the requests are parsed, before any engine pass."""
    from lmms_owc_amd.models import get_model
    from lmms_owc_amd.tasks import load_task

    outs = {}
    for bs in (1, 4):
        task = load_task("synthetic:8:70x120:3")
        lm = get_model("custom-model", model_type=model_type, model_name_or_path=f"synthetic:{name}", kv_dtype="fp8", batch_size=bs)
        lm.task_dict[task.task_name] = task.dataset
        task.build_all_requests(limit=None, rank=0, world_size=1)
        outs[bs] = lm.generate_until(task.instances)
    assert outs[1] == outs[4] and len(outs[4]) == 8 and all(isinstance(s, str) for s in outs[4])
    assert lm.model.d.kv_dtype == "fp8" and lm.model._kv[0].dtype == torch.uint8
    with pytest.raises(ValueError, match="kv_dtype"):
        get_model("custom-model", model_type=model_type, model_name_or_path=f"synthetic:{name}", kv_dtype="fp4")
    task = load_task("synthetic:3:70x120:3")
    task.generation_kwargs.update({"num_beams": 2})
    task.build_all_requests(limit=None, rank=0, world_size=1)
    lm.task_dict[task.task_name] = task.dataset
    eng = lm.model

    def no_pass(*a, **kw):
        raise AssertionError("an engine pass ran")

    eng.generate = eng.generate_beam = eng.encode_images = no_pass
    with pytest.raises(ValueError, match="kv_dtype=fp8"):
        lm.generate_until(task.instances)
