"""Straggler hand-over between the passes of a task under a repetition penalty: the seen-token bitmap row of an unfinished
sequence travels with it (`carry["out"]["seen"]`, `Qwen2VLEngine.generate`), so a sequence's tokens do not depend on the pass
that finishes it - for the bf16 and the fp8 cache, forced / free-running / sampled, through more than one hop
(test_the_imported_rows_decide_the_tokens ends 32 sequences that two passes handed on).

Tiny decoder of tests/test_qwen2vl_gpu.py (2 layers, d_model 256, vocab 512: a bitmap row is 16 words), text-only prompts.
Everything here is token EQUALITY between two runs of the same kernels (batch invariance): no tolerance is involved.
"""
import numpy as np
import pytest
import torch

from tests import recipes
from tests.util import to_np

pytestmark = pytest.mark.gpu
KW = dict(v_depth=2, v_embed=160, v_heads=2, v_mlp=640, n_layers=2, d_model=256, n_q_heads=2, n_kv_heads=1, d_ff=512, vocab=512,
          tie_embeddings=False, image_token_id=500, max_positions=512, max_grid=64)
WPR = 16                                                   # words of a bitmap row: vocab 512 / 32


@pytest.fixture(scope="module")
def setup(gpu):
    from lmms_owc_amd.engine.qwen2vl import Qwen2VLDims, Qwen2VLEngine, Qwen2VLWeights

    w = recipes.qwen2vl_weights(recipes.tiny_cfg(), 1234)
    eng = Qwen2VLEngine(Qwen2VLWeights.from_state_dict(Qwen2VLDims(**KW), w, gpu), vit_chunk_tokens=64, prefill_chunk_tokens=40)
    eng8 = Qwen2VLEngine(Qwen2VLWeights.from_state_dict(Qwen2VLDims(**KW, kv_dtype="fp8"), w, gpu))
    return eng, eng8


def _ragged_forced(rng, B, T, eos, vocab, mean_len, cap_frac=0.02):
    """Seeded per-sequence continuations: geometric stop lengths (a few forced to the cap), EOS at the stop column."""
    lens = np.minimum(rng.geometric(1.0 / mean_len, B), T)
    lens[rng.random(B) < cap_frac] = T + 1                       # never stops inside the cap
    forced = rng.integers(1, vocab, (B, T))
    forced[forced == eos] = eos - 1
    for b in range(B):
        if lens[b] <= T:
            forced[b, lens[b] - 1] = eos
    return forced.astype(np.int32), lens


def _none(p):
    return [[] for _ in p]


def _frequent(tokens) -> int:
    vals, counts = np.unique(tokens, return_counts=True)
    return int(vals[np.argmax(counts)])


def _ids(row) -> set:
    """The token ids marked in one bitmap row (int32 words, bit i of word w = id 32 w + i)."""
    bits = np.unpackbits(row.detach().cpu().contiguous().numpy().view(np.uint8), bitorder="little")
    return set(np.flatnonzero(bits).tolist())


def run_passes(eng, passes, caps, eos, below, penalty, *, forced=None, sampling=None, between=None):
    """The passes of a task with the hand-over on: (tokens by (pass, index), number of exports, the exported states)."""
    got, state, handed, states = {}, None, 0, []
    for k, p in enumerate(passes):
        c = {"in": state, "below": below if k + 1 < len(passes) else 0, "tags": [(k, i) for i in range(len(p))]}
        out = to_np(eng.generate(p, None, _none(p), caps[k], eos_token_id=eos, pad_token_id=0, carry=c, repetition_penalty=penalty,
                                 forced_tokens=None if forced is None else forced[k], sampling=None if sampling is None else sampling[k]))
        got.update({(k, i): out[i] for i in range(len(p)) if i not in c["unfinished_rows"]})
        got.update(dict(c["finished"]))
        state = c["out"]
        states.append(state)
        handed += 0 if state is None else len(state["tags"])
        if state is not None and between is not None:
            between(state)
    assert state is None and len(got) == sum(len(p) for p in passes)
    return got, handed, states


SIZES, CAPS = (70, 50, 33, 21), (40, 24, 40, 32)   # passes of different generation lengths: a carried sequence keeps ITS cap


@pytest.fixture(scope="module")
def four_passes():
    r = np.random.default_rng(123)
    passes = [[r.integers(10, 400, 6 + (i % 9)).astype(np.int64) for i in range(n)] for n in SIZES]
    forced = [_ragged_forced(r, n, T, 9, 400, 6, cap_frac=0.08)[0] for n, T in zip(SIZES, CAPS)]
    return passes, forced


@pytest.mark.parametrize("mode,below,at_least", [("forced", 6, 6), ("free", 40, 10), ("sampled", 40, 10)])
def test_a_carried_sequence_equals_the_one_finished_in_one_pass_under_a_penalty(setup, four_passes, mode, below, at_least):
    """Four passes of 70 / 50 / 33 / 21 prompts, caps 40 / 24 / 40 / 32, repetition penalty 1.3 (the layout of
    test_straggler_carry_over_is_bit_identical): every sequence's tokens equal those of its pass run alone to its end under the
    same penalty; sequences really travel (observed on MI355X: 8 forced, 33 free-running, 32 sampled; before the bitmap travelled
    the engine ran every pass to its end under a penalty and the count was 0); the penalty really changes the tokens (31 / 156 /
    172 of the 174 sequences)."""
    eng, _ = setup
    passes, forced = four_passes
    pen = 1.3
    smp = None
    if mode == "sampled":
        smp = [{"temperature": 0.9, "top_k": 30, "seed": 11, "stream_ids": 1000 * k + np.arange(len(p))} for k, p in enumerate(passes)]
    fo = forced if mode == "forced" else None
    eos = 9
    if mode != "forced":   # an EOS that ends many sequences early and some never: the most frequent token of the PENALISED free run
        eos = _frequent(to_np(eng.generate(passes[0], None, _none(passes[0]), CAPS[0], repetition_penalty=pen))[:, 2:20])

    def alone(penalty):
        return [to_np(eng.generate(p, None, _none(p), CAPS[k], eos_token_id=eos, pad_token_id=0, repetition_penalty=penalty,
                                   forced_tokens=None if fo is None else fo[k], sampling=None if smp is None else smp[k]))
                for k, p in enumerate(passes)]

    ref, plain = alone(pen), alone(1.0)
    changed = sum(int(not np.array_equal(a, b)) for x, y in zip(ref, plain) for a, b in zip(x, y))
    got, handed, states = run_passes(eng, passes, CAPS, eos, below, pen, forced=fo, sampling=smp)
    # per pass: how many sequences it exported, by the pass they started in (an earlier pass = carried through more than one hop)
    exports = [{} if s is None else {k0: sum(1 for t in s["tags"] if t[0] == k0) for k0 in range(k + 1)} for k, s in enumerate(states)]
    print(f"[penalty hand-over] {mode}: eos {eos}, {handed} sequences handed over (per pass, by pass of origin: {exports}), "
          f"{changed} of {sum(SIZES)} sequences differ from the unpenalised run")
    for s in states:
        if s is not None:
            assert s["penalty"] == pen and s["seen"].shape == (len(s["tags"]), WPR) and s["seen"].dtype == torch.int32
    for k, n in enumerate(SIZES):
        for i in range(n):
            assert np.array_equal(got[(k, i)], ref[k][i]), (mode, k, i, got[(k, i)], ref[k][i])
    assert handed >= at_least, handed
    assert changed > 0


def test_the_imported_rows_decide_the_tokens(setup):
    """Two passes at penalty 2.0; the second one's prompts share a leading text (the prefill's shared-prefix broadcast).  With the
    exported state untouched every sequence equals its pass run alone; with `state["seen"]` zeroed between the passes the carried
    sequences lose their history and at least 3 of them continue differently (observed on MI355X: 22 of 34).  And hop by hop: a sequence's exported row is its
    prompt's ids plus the ids it was FED (the pending token is not in it), and after a second hop the first row plus exactly what
    it was fed in between - none of the second pass's prefix ids."""
    eng, _ = setup
    pen, cap = 2.0, 24
    r = np.random.default_rng(2024)
    first = [r.integers(10, 400, 6 + (i % 9)).astype(np.int64) for i in range(40)]
    head = np.arange(440, 449)                           # ids no prompt of the first pass holds
    second = [np.concatenate([head, r.integers(10, 400, 3 + (i % 5))]).astype(np.int64) for i in range(20)]
    assert eng.share_prefix and eng._common_prefix(second, 0, 2) == len(head)
    passes = [first, second]
    eos = _frequent(to_np(eng.generate(first, None, _none(first), cap, repetition_penalty=pen))[:, 2:20])
    ref = [to_np(eng.generate(p, None, _none(p), cap, eos_token_id=eos, pad_token_id=0, repetition_penalty=pen)) for p in passes]

    got, handed, states = run_passes(eng, passes, (cap, cap), eos, 34, pen)
    carried = [t for t in states[0]["tags"]]
    assert handed == len(carried) >= 6, handed
    for k, p in enumerate(passes):
        for i in range(len(p)):
            assert np.array_equal(got[(k, i)], ref[k][i]), (k, i)
    wiped, _, _ = run_passes(eng, passes, (cap, cap), eos, 34, pen, between=lambda s: s["seen"].zero_())
    differ = [t for t in carried if not np.array_equal(wiped[t], ref[t[0]][t[1]])]
    print(f"[penalty hand-over] eos {eos}: {len(carried)} carried sequences, {len(differ)} differ once their bitmap rows are zeroed")
    assert len(differ) >= 3, (len(differ), len(carried))
    for i in range(len(second)):                          # the pass's own sequences never read those rows
        assert np.array_equal(wiped[(1, i)], ref[1][i]), i

    # hop by hop: export after pass 1, import into pass 2, export again while pass 2 still has many live sequences
    c1 = {"in": None, "below": 34, "tags": [(0, i) for i in range(len(first))]}
    eng.generate(first, None, _none(first), cap, eos_token_id=eos, pad_token_id=0, carry=c1, repetition_penalty=pen)
    s1 = c1["out"]
    c2 = {"in": s1, "below": len(second), "tags": [(1, i) for i in range(len(second))]}   # (stops at its first look at the flags)
    eng.generate(second, None, _none(second), cap, eos_token_id=eos, pad_token_id=0, carry=c2, repetition_penalty=pen)
    s2 = c2["out"]
    twice = [t for t in s2["tags"] if t[0] == 0]
    assert len(twice) >= 3, len(twice)
    for t in twice:
        a, b = s1["tags"].index(t), s2["tags"].index(t)
        tok1, tok2 = s1["tokens"][a], s2["tokens"][b]
        assert len(tok2) > len(tok1) and np.array_equal(tok2[:len(tok1)], tok1)
        row1, row2 = _ids(s1["seen"][a]), _ids(s2["seen"][b])
        assert row1 == set(first[t[1]].tolist()) | set(tok1[:-1].tolist()), t           # prompt + fed tokens; the pending one is not marked
        fed = set(tok2[len(tok1) - 1:-1].tolist())                                      # the pending token of hop 1 .. the last one fed
        assert row2 == row1 | fed, (t, sorted(row2 - row1 - fed), sorted((row1 | fed) - row2))
        only_prefix = set(head.tolist()) - row1 - fed
        assert only_prefix and not (only_prefix & row2), t
    own = [t for t in s2["tags"] if t[0] == 1]                                          # the pass's own rows DO hold the prefix
    assert own and all(set(head.tolist()) <= _ids(s2["seen"][s2["tags"].index(t)]) for t in own)
    # a third pass ends them all: a sequence carried through two hops still equals its own pass run alone
    third = [r.integers(10, 400, 7 + i).astype(np.int64) for i in range(5)]
    c3 = {"in": s2, "below": 0, "tags": [(2, i) for i in range(len(third))]}
    eng.generate(third, None, _none(third), cap, eos_token_id=eos, pad_token_id=0, carry=c3, repetition_penalty=pen)
    done = dict(c3["finished"])
    assert c3["out"] is None and set(done) == set(s2["tags"])
    for t in s2["tags"]:
        assert np.array_equal(done[t], ref[t[0]][t[1]]), t
    print(f"[penalty hand-over] {len(twice)} sequences went through two hops, {len(own)} of the second pass through one")


def test_fp8_cache_twin(setup):
    """40 + 20 prompts, cap 24, hand-over once at most 37 own sequences run, fp8 cache, penalty 1.3 (the layout of
    tests/test_kv_fp8_model_gpu.py::test_a_carried_sequence_equals_the_one_finished_in_one_pass): codes, scales AND bitmap rows
    (observed on MI355X: 36 sequences handed over)."""
    _, e8 = setup
    pen = 1.3

    def prompts(n, seed):
        r = np.random.default_rng(seed)
        return [r.integers(1, 490, 12 + (i % 7)).astype(np.int64) for i in range(n)]

    passes = [prompts(40, 21), prompts(20, 22)]
    eos = _frequent(to_np(e8.generate(passes[0], None, _none(passes[0]), 24, repetition_penalty=pen))[:, 2:20])
    ref = [to_np(e8.generate(p, None, _none(p), 24, eos_token_id=eos, pad_token_id=0, repetition_penalty=pen)) for p in passes]
    plain = to_np(e8.generate(passes[0], None, _none(passes[0]), 24, eos_token_id=eos, pad_token_id=0, repetition_penalty=1.0))
    got, handed, states = run_passes(e8, passes, (24, 24), eos, 37, pen)
    print(f"[penalty hand-over] fp8 cache: eos {eos}, {handed} sequences handed over")
    s = states[0]
    assert s is not None and len(s["kv_scales"]) == 2 and s["k"].dtype == torch.uint8
    assert s["seen"] is not None and s["seen"].shape == (len(s["tags"]), WPR) and s["penalty"] == pen
    assert handed >= 3, handed
    for k, p in enumerate(passes):
        for i in range(len(p)):
            assert np.array_equal(got[(k, i)], ref[k][i]), (k, i)
    assert not np.array_equal(ref[0], plain)


def test_mismatched_carried_state_is_refused(setup):
    """A pass takes carried-in sequences only at their own penalty and bitmap row width: each mismatch is a ValueError naming both
    values, and the context's penalty option is off afterwards (a plain `generate` on the same engine gives the plain tokens)."""
    eng, _ = setup
    r = np.random.default_rng(77)
    first = [r.integers(10, 400, 6 + (i % 9)).astype(np.int64) for i in range(12)]
    second = [r.integers(10, 400, 6 + (i % 5)).astype(np.int64) for i in range(5)]
    eos = 511                                            # far outside the prompts' ids: rarely emitted, so sequences stay alive
    plain = to_np(eng.generate(second, None, _none(second), 6))

    def export(penalty):
        c = {"in": None, "below": 12, "tags": list(range(len(first)))}
        eng.generate(first, None, _none(first), 8, eos_token_id=eos, pad_token_id=0, carry=c, repetition_penalty=penalty)
        assert c["out"] is not None and len(c["out"]["tags"]) >= 3
        return c["out"]

    with_pen, without = export(1.3), export(1.0)
    assert with_pen["penalty"] == 1.3 and with_pen["seen"].shape[1] == WPR
    assert without["penalty"] == 1.0 and without["seen"] is None
    wide = {**with_pen, "seen": torch.cat([with_pen["seen"], torch.zeros_like(with_pen["seen"][:, :1])], dim=1)}
    cases = [(with_pen, 1.0, r"1\.3.*1\.0"), (without, 1.3, r"1\.3.*1\.0"), (with_pen, 1.5, r"1\.3.*1\.5"), (wide, 1.3, r"17.*16")]
    for state, penalty, names in cases:
        c = {"in": state, "below": 0, "tags": list(range(len(second)))}
        with pytest.raises(ValueError, match=names):
            eng.generate(second, None, _none(second), 6, eos_token_id=eos, pad_token_id=0, carry=c, repetition_penalty=penalty)
        assert np.array_equal(to_np(eng.generate(second, None, _none(second), 6)), plain), penalty
    # ... and the matching state is accepted
    c = {"in": with_pen, "below": 0, "tags": list(range(len(second)))}
    eng.generate(second, None, _none(second), 6, eos_token_id=eos, pad_token_id=0, carry=c, repetition_penalty=1.3)
    assert c["out"] is None and len(c["finished"]) == len(with_pen["tags"])


def test_the_bitmap_outlives_the_decode_loop(setup, gpu, monkeypatch):
    """The context reads and writes the bitmap through a raw pointer for the whole call, so the engine must hold the tensor for the
    whole call.  Once the first decode step has been enqueued, every `_i32` upload here also allocates four device tensors of exactly
    the bitmap's size, fills them with 0xFF and keeps them until the upload returns: were the bitmap's block back in torch's
    caching allocator by then, one of them would land in it and every id would read as seen.  The compacting run uploads inside
    the loop (the list of live rows), the other one does not: their tokens must be equal."""
    eng, _ = setup
    pen = 1.3
    r = np.random.default_rng(9)
    prompts = [r.integers(10, 400, 6 + (i % 9)).astype(np.int64) for i in range(48)]
    none = _none(prompts)
    eos = _frequent(to_np(eng.generate(prompts, None, none, 24, repetition_penalty=pen))[:, 2:20])
    kw = dict(eos_token_id=eos, pad_token_id=0, stop_check_every=1, repetition_penalty=pen)
    st = {}
    want = to_np(eng.generate(prompts, None, none, 24, compact_rows=True, stats=st, **kw))
    assert min(st["live_rows_per_step"]) < len(prompts)               # rows really leave the batch: the loop compacts
    nbytes = len(prompts) * WPR * 4                                   # one row per slot; without `carry` a pass has one slot per prompt
    seen = {"stepped": False, "extra": 0}
    step, i32 = eng._lib.owc_llm_decode_step, eng._i32

    def step_spy(*a):
        rc = step(*a)
        seen["stepped"] = True
        return rc

    def i32_spy(a):
        extra = []
        if seen["stepped"]:
            extra = [torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=gpu) for _ in range(4)]
            seen["extra"] += 1
        out = i32(a)
        del extra
        return out

    monkeypatch.setattr(eng._lib, "owc_llm_decode_step", step_spy)
    monkeypatch.setattr(eng, "_i32", i32_spy)
    runs = {}
    for compact in (True, False):
        seen["stepped"] = False
        runs[compact] = to_np(eng.generate(prompts, None, none, 24, compact_rows=compact, **kw))
        if compact:
            assert seen["extra"] > 0                                  # the wrapper did allocate inside the loop
    assert np.array_equal(runs[True], runs[False])
    assert np.array_equal(runs[True], want)
