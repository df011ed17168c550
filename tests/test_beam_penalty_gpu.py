"""Beam search under the checkpoint's repetition penalty on the GPU.

HF's beam search applies RepetitionPenaltyLogitsProcessor to the LOG-SOFTMAX output: every id a hypothesis has seen (its prompt,
image placeholders included, and its own generated tokens) gets lp < 0 ? lp * p : lp / p before the candidates are ranked.
Device: `owc_beam_candidates_penalized` reads the seen-token bitmap row of each running beam's cache slot; host: `generate_beam`
keeps the bitmap rows with the hypotheses as it keeps their K / V rows.  Checked against numpy (the op), against
tests/beam_penalty_ref.py driven by the engine's own logits (the engine; the restatement is pinned on HF in
tests/test_oracle_beam_penalty.py), through the model plug-ins, and for the context option being cleared afterwards."""
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import recipes
from tests.beam_penalty_ref import beam_search_penalized
from tests.util import to_np

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).parent / "golden"


# ---- the op -------------------------------------------------------------------------------------------------------------
def _ref_candidates(x: np.ndarray, logz: np.ndarray, seen_bits: np.ndarray, row_slot: np.ndarray, p: float, k: int):
    """numpy: fp32(l) - logz (the device's logz), penalised where the bitmap row row_slot[r] has the id, top k by (value desc, id)."""
    rows, V = x.shape
    lp = (x.astype(np.float32) - logz.astype(np.float32)[:, None]).astype(np.float32)
    hit = seen_bits[row_slot][:, :V]
    p32 = np.float32(p)
    v = np.where(hit, np.where(lp < 0, lp * p32, lp / p32), lp).astype(np.float32)
    order = np.lexsort((np.broadcast_to(np.arange(V), v.shape), -v.astype(np.float64)), axis=-1)[:, :k]
    return np.take_along_axis(v, order, -1), order, v


def _bitmap(bits: np.ndarray) -> torch.Tensor:
    """bool [slots, words * 32] -> the int32 [slots, words] bitmap the library reads (little endian: id i = bit i % 32 of word i / 32)."""
    w = np.packbits(bits, axis=-1, bitorder="little")
    return torch.from_numpy(w.view(np.uint32).view(np.int32).copy())


@pytest.mark.parametrize("V", [97, 1000, 152064])
@pytest.mark.parametrize("k", [1, 6, 64])
def test_penalized_candidates_vs_numpy(gpu, V, k):
    """Rows of bf16 logits in a wider buffer (ld > vocab, the padding columns hold values that would win), bitmap rows picked through a
    non-identity row_slot, seen sets that cover a row's whole unpenalised top k, planted ties - equal logits, and at p = 2 a seen id
    whose penalised log-prob equals an unseen id's - against numpy on the same bf16 values and the device's logz; at p = 1 the
    result is `owc_beam_candidates` bit for bit (logz, ids, and values = fp32(logit - logz))."""
    from lmms_owc_amd import ops

    rng = np.random.default_rng(V * 100 + k)
    rows, slots, ld = 6, 9, V + 13
    buf = torch.full((rows, ld), 3.0e4, dtype=torch.bfloat16)            # padding columns: larger than every logit
    x = torch.from_numpy((rng.normal(size=(rows, V)) * 3).astype(np.float32)).to(torch.bfloat16)
    x[1, : V // 2] = x[1, V // 2: V // 2 * 2]                            # planted ties among equal logits, also at the top
    x[3] = 1.5                                                            # a constant row
    # row 4: logz = 100 exactly (one logit 100, every other exp underflows), so lp = l - 100 is exact and at p = 2 the seen id 2
    # (l = -28: lp -128 -> -256) ties the unseen id 5 (l = -156: lp -256); id 1 and id 7 tie at l = -30 (one seen, one not)
    x[4] = -170.0
    x[4, 3], x[4, 2], x[4, 5], x[4, 1], x[4, 7] = 100.0, -28.0, -156.0, -30.0, -30.0
    buf[:, :V] = x
    f = x.float().numpy()
    row_slot = np.array([4, 0, 8, 2, 6, 4], np.int32)                    # slot 4 read by two rows, slots 1 3 5 7 by none
    bits = np.zeros((slots, (V + 31) // 32 * 32), bool)
    for s in range(slots):
        bits[s, rng.integers(0, V, max(1, V // 10))] = True
    raw_top = np.lexsort((np.broadcast_to(np.arange(V), f.shape), -f.astype(np.float64)), axis=-1)[:, : min(V, 2 * k + 2)]
    bits[row_slot[0], raw_top[0]] = True                                 # the whole unpenalised top of rows 0 and 2 is seen
    bits[row_slot[2], raw_top[2]] = True
    bits[row_slot[4], :] = False
    bits[row_slot[4], [2, 1]] = True
    seen = _bitmap(bits).to(gpu)
    xg, slot_t = buf.to(gpu)[:, :V], torch.from_numpy(row_slot).to(gpu)
    assert xg.stride(0) == ld

    lz0, tv0, ti0 = (to_np(t) for t in ops.beam_candidates(xg, k))
    for p in (0.8, 1.05, 1.3, 2.0):
        logz, tv, ti = (t.cpu().numpy() for t in ops.beam_candidates_penalized(xg, k, seen, p, slot_t))
        assert np.array_equal(logz.view(np.int32), lz0.view(np.int32)), p           # the same log-sum-exp, bit for bit
        want_v, want_i, v = _ref_candidates(f, logz, bits, row_slot, p, k)
        assert np.array_equal(ti, want_i), (p, ti, want_i)
        assert np.array_equal(tv.view(np.int32), want_v.view(np.int32)), p
        if p == 2.0:
            assert logz[4] == 100.0 and v[4, 2] == v[4, 5] == -256.0             # the seen / unseen tie is really planted
            if k >= 6:   # 0, -130 (unseen 7), -256 (seen 2, unseen 5: the lower id first), -260 (seen 1), then -270 from id 0 on
                assert list(ti[4, :6]) == [3, 7, 2, 5, 1, 0], ti[4, :6]
    m = f.max(-1).astype(np.float64)
    want_z = m + np.log(np.exp(f.astype(np.float64) - m[:, None]).sum(-1))
    np.testing.assert_allclose(lz0, want_z, rtol=0, atol=2e-5 * max(1.0, np.abs(want_z).max()))

    # penalty 1: owc_beam_candidates exactly
    logz, tv, ti = (t.cpu().numpy() for t in ops.beam_candidates_penalized(xg, k, seen, 1.0, slot_t))
    assert np.array_equal(logz.view(np.int32), lz0.view(np.int32))
    assert np.array_equal(ti, ti0)
    assert np.array_equal(tv.view(np.int32), (tv0 - lz0[:, None]).astype(np.float32).view(np.int32))
    # identity row_slot (None) == an explicit arange
    a = [to_np(t) for t in ops.beam_candidates_penalized(xg, k, seen[:rows].contiguous(), 1.3)]
    b = [to_np(t) for t in ops.beam_candidates_penalized(xg, k, seen, 1.3, torch.arange(rows, dtype=torch.int32, device=gpu))]
    assert all(np.array_equal(u, w) for u, w in zip(a, b))


def test_penalized_candidates_refuses_bad_arguments(gpu):
    from lmms_owc_amd import _lib, ops

    x = torch.zeros((2, 1000), dtype=torch.bfloat16, device=gpu)
    seen = torch.zeros((2, 32), dtype=torch.int32, device=gpu)
    with pytest.raises(_lib.OwcError):
        ops.beam_candidates_penalized(x, 65, seen, 1.3)                   # k > 64
    with pytest.raises(_lib.OwcError):
        ops.beam_candidates_penalized(x, 4, seen[:, :31].contiguous(), 1.3)   # 31 * 32 < 1000: bitmap too narrow
    with pytest.raises(_lib.OwcError):
        ops.beam_candidates_penalized(x, 4, seen, 0.0)                    # penalty must be > 0
    ops.beam_candidates_penalized(x, 4, seen, 1.3)
    torch.cuda.synchronize()


# ---- the engine ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def setup(gpu):
    from lmms_owc_amd.engine.qwen2vl import Qwen2VLDims, Qwen2VLEngine, Qwen2VLWeights

    cfg = recipes.tiny_cfg()
    w = recipes.qwen2vl_weights(cfg, 1234)
    dims = Qwen2VLDims(v_depth=2, v_embed=160, v_heads=2, v_mlp=640, n_layers=2, d_model=256, n_q_heads=2, n_kv_heads=1,
                       d_ff=512, vocab=512, tie_embeddings=False, image_token_id=500, max_positions=512, max_grid=64)
    make = lambda: Qwen2VLEngine(Qwen2VLWeights.from_state_dict(dims, w, gpu), vit_chunk_tokens=64, prefill_chunk_tokens=40)  # noqa: E731
    return cfg, make(), make, np.load(GOLD / "qwen2vl_tiny.npz")


def _engine_logits_fn(eng, prompt, emb, grid, rows):
    """next-token RAW logits of prompt + each continuation, every one recomputed from the prompt (teacher forcing, no penalty;
    memoised: the searches of one prompt under several EOS ids ask for the same continuations)."""
    memo = {}

    def fn(conts):
        key = tuple(tuple(int(t) for t in c) for c in conts)
        if key not in memo:
            gl = len(conts[0])
            forced = np.zeros((len(conts), gl + 1), np.int64)
            forced[:, :gl] = np.asarray(conts, np.int64).reshape(len(conts), gl)
            _, lg = eng.generate([prompt] * len(conts), emb, [grid] * len(conts), gl + 1,
                                 img_rows=None if rows is None else [rows] * len(conts), forced_tokens=forced, return_step_logits=True,
                                 repetition_penalty=1.0)
            memo[key] = lg[gl].float().cpu().numpy()
        return memo[key]
    return fn


@pytest.mark.parametrize("k,T", [(2, 6), (3, 8), (4, 7)])
def test_penalised_beam_search_equals_the_restatement_on_the_engines_logits(setup, gpu, k, T):
    """`generate_beam(repetition_penalty=p)` against tests/beam_penalty_ref.py fed the engine's own logits: the same tokens (the
    bitmap rows must follow the hypotheses, image placeholders must count as seen), scores within fp32 rounding of the two
    log-sum-exps; one prompt alone = the same prompt in the batch; the penalty changes at least one answer."""
    cfg, eng, _, g = setup
    grid = [(1, 4, 4)]
    emb = eng.encode_images(torch.from_numpy(recipes.pixel_values(grid, 7)).to(torch.bfloat16).to(gpu), grid)
    n_img = emb.shape[0]
    rng = np.random.default_rng(1000 * k + T)
    base = rng.integers(1, 480, 6)
    prompts = [np.asarray(g["a_ids"]), rng.integers(1, 480, 9).astype(np.int64), np.concatenate([base, base, base[:3]]).astype(np.int64),
               np.asarray(g["a_ids"])[:-2], rng.integers(1, 480, 17)]
    grids = [grid if (p == 500).any() else [] for p in prompts]
    rows = [np.arange(n_img) if (p == 500).any() else np.zeros(0, np.int64) for p in prompts]
    fns = [_engine_logits_fn(eng, prompts[b], emb, grids[b], rows[b]) for b in range(len(prompts))]
    plain = to_np(eng.generate_beam(prompts, emb, grids, T, k, eos_token_id=-1, pad_token_id=0, img_rows=rows)).astype(int)
    differs = False
    for p in (1.3, 1.05):
        free = to_np(eng.generate_beam(prompts, emb, grids, T, k, eos_token_id=-1, pad_token_id=0, img_rows=rows,
                                       repetition_penalty=p)).astype(int)
        for eos in (int(free[0, 2]), int(free[2, min(3, T - 1)]), -1):
            want = [beam_search_penalized(fns[b], prompts[b], k, T, eos, 0, repetition_penalty=p) for b in range(len(prompts))]
            got, scores = eng.generate_beam(prompts, emb, grids, T, k, eos_token_id=eos, pad_token_id=0, img_rows=rows,
                                            return_scores=True, repetition_penalty=p)
            got = to_np(got).astype(int)
            for b in range(len(prompts)):
                assert np.array_equal(got[b], want[b][0]), (k, T, p, eos, b, got[b], want[b][0])
                assert abs(scores[b] - want[b][1]) < 2e-3 * max(1.0, abs(want[b][1])), (p, eos, b, scores[b], want[b][1])
            alone = to_np(eng.generate_beam(prompts[2:3], emb, grids[2:3], T, k, eos_token_id=eos, pad_token_id=0, img_rows=rows[2:3],
                                            repetition_penalty=p)).astype(int)
            assert np.array_equal(alone[0], got[2]), (p, eos)
        differs |= bool((free != plain).any())
    assert differs, "the penalty changed no beam answer on this model: the test would not see a missing penalty"
    # the engine attribute (what a plug-in sets from generation_config.json) is the default of the keyword
    eng.repetition_penalty = 1.3
    try:
        via_attr = to_np(eng.generate_beam(prompts, emb, grids, T, k, eos_token_id=-1, pad_token_id=0, img_rows=rows)).astype(int)
    finally:
        eng.repetition_penalty = 1.0
    assert np.array_equal(via_attr, to_np(eng.generate_beam(prompts, emb, grids, T, k, eos_token_id=-1, pad_token_id=0, img_rows=rows,
                                                               repetition_penalty=1.3)).astype(int))


def test_penalised_beam_search_at_decoder_widths(gpu):
    """Two decoder layers at Qwen2-VL-7B widths (3584 / 28 q / 4 kv heads / 18944, vocabulary 152064): the candidates kernel at its
    production row length, the bitmap at 4752 words a row; text prompts with repeated ids; tokens equal to the restatement fed the
    engine's own logits."""
    from lmms_owc_amd.engine.qwen2vl import Qwen2VLDims, Qwen2VLEngine, Qwen2VLWeights

    dims = Qwen2VLDims(v_depth=1, v_embed=160, v_heads=2, v_mlp=640, n_layers=2, max_positions=512, max_grid=64)
    eng = Qwen2VLEngine(Qwen2VLWeights.random(dims, gpu, seed=77))
    rng = np.random.default_rng(3)
    head = rng.integers(1, 150000, 7)
    prompts = [np.concatenate([head, head[:4], rng.integers(1, 150000, 5)]).astype(np.int64), rng.integers(1, 150000, 12).astype(np.int64)]
    k, T, p = 3, 6, 1.3
    got = to_np(eng.generate_beam(prompts, None, [[], []], T, k, eos_token_id=-1, pad_token_id=0, repetition_penalty=p)).astype(int)
    for b in range(2):
        want, _ = beam_search_penalized(_engine_logits_fn(eng, prompts[b], None, [], None), prompts[b], k, T, -1, 0, repetition_penalty=p)
        assert np.array_equal(got[b], want), (b, got[b], want)


def test_context_option_cleared_after_a_penalised_beam_call(setup, gpu):
    """After `generate_beam` with a penalty the context holds no bitmap: a greedy `generate(repetition_penalty=1.0)` on the same engine
    is bit-identical (tokens and every step's logits) to the same call on a fresh engine."""
    cfg, eng, make, g = setup
    rng = np.random.default_rng(8)
    prompts = [rng.integers(1, 480, 10 + 3 * i).astype(np.int64) for i in range(3)]
    eng.generate_beam(prompts, None, [[]] * 3, 6, 3, eos_token_id=-1, pad_token_id=0, repetition_penalty=1.3)
    ta, la = eng.generate(prompts, None, [[]] * 3, 6, return_step_logits=True, repetition_penalty=1.0)
    tb, lb = make().generate(prompts, None, [[]] * 3, 6, return_step_logits=True, repetition_penalty=1.0)
    assert torch.equal(ta, tb) and torch.equal(la, lb)


# ---- the plug-ins -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model_type", ["qwen2-vl", "llava"])
def test_num_beams_under_the_checkpoint_penalty_through_the_plugin(gpu, model_type):
    """`--gen_kwargs num_beams=3` on a model whose generation_config.json carries repetition_penalty 1.3 (set on the engine, as
    `Qwen2VL.load_model` does): every engine call the plug-in makes equals the engine-level call with `repetition_penalty=1.3`, the
    answers do not depend on the batch size, and they differ from the unpenalised beams."""
    from lmms_owc_amd.models import get_model
    from lmms_owc_amd.tasks import load_task

    outs = {}
    for tag, bs, rep in (("plain", 4, 1.0), ("b1", 1, 1.3), ("b4", 4, 1.3)):
        task = load_task("synthetic:7:56x84:3")
        task.generation_kwargs.update({"num_beams": 3})
        task.build_all_requests(limit=None, rank=0, world_size=1)
        lm = get_model("custom-model", model_type=model_type, model_name_or_path="synthetic:tiny", batch_size=bs)
        lm.task_dict[task.task_name] = task.dataset
        eng = lm._model
        eng.repetition_penalty = rep
        calls = []
        orig = eng.generate_beam

        def spy(*a, _orig=orig, _calls=calls, **kw):
            out = _orig(*a, **kw)
            _calls.append((a, kw, out.clone()))
            return out

        eng.generate_beam = spy
        outs[tag] = lm.generate_until(task.instances)
        assert calls and all(c[0][4] == 3 for c in calls)
        if rep != 1.0:
            for a, kw, out in calls:
                assert torch.equal(orig(*a, **{**kw, "repetition_penalty": rep}), out)
    assert outs["b1"] == outs["b4"] and len(outs["b4"]) == 7
    assert outs["b4"] != outs["plain"], "the penalty changed no answer through the plug-in"
