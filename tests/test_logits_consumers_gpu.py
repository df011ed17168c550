"""The kernels that read a row of bf16 logits - penalty write-back, sampler, argmax, beam candidates, token log-probability - each
against a plain numpy reference of the same operation, at the row widths of the real vocabularies and at ragged ones, with strided
rows inside guard bands.

References: `oracle.qwen2vl_np.repetition_penalty_scores` and `oracle.sampling_np.sampling_probs` (both pinned on the installed
transformers' own processors in tests/test_oracle_sampling.py, where the order of the chain is pinned too) and `np_ops.bf16_round`.
The library is built without fast-math: an fp32 multiply, an fp32 divide and a round-to-nearest-even are exactly rounded on both
sides, so the write-back is compared BIT FOR BIT.
"""
import numpy as np
import pytest
import torch

from oracle import np_ops
from oracle import qwen2vl_np as Q
from oracle import sampling_np as S
from tests.penalty_cases import CONFIGS, host_bitmap, sampling_row, shipped_config_rows
from tests.util import CANARY, POISON, assert_guard_intact, assert_same_bits, embed, guarded, to_np

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


def i32(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(gpu)


def dev_bitmap(bits, gpu):
    return torch.from_numpy(bits.view(np.int32).copy()).to(gpu)


def bf16_t(x):
    """float32 numpy values that are bf16-representable -> bf16 tensor holding exactly those bits (signed zeros included)."""
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(BF16)


def odd_strided(t, ld, fill):
    """`t` [rows, V] copied into a view of row stride `ld` (ANY value > V, odd ones included - tests.util.guarded keeps leading
    dimensions at multiples of 16 bytes) inside a 1-D backing buffer filled with `fill`: 300 fill cells in front, the gaps between
    the rows, 300 + ld cells behind.  Returns (backing, view)."""
    rows, V = t.shape
    assert ld > V
    backing = torch.empty(300 + rows * ld + 300, dtype=t.dtype, device=t.device)
    backing.view(torch.int16).fill_(fill if fill < 0x8000 else fill - 0x10000)
    view = backing.as_strided((rows, V), (ld, 1), 300)
    view.copy_(t)
    return backing, view


# ---- a. the penalty write-back, bit for bit -----------------------------------------------------------------------------------------
def _writeback_case(V, seed):
    """6 rows of logits (positive, negative, +0 and -0 among the seen AND the unseen columns) and 3 histories: ids 0, 31, 32, V - 1, the
    ids on each side of every 1024-word stride of the kernel's loop (one thread owns words t, t + 1024, ...), ~2000 random ones."""
    r = np.random.default_rng(seed)
    x = np_ops.bf16_round((r.standard_normal((6, V)) * 4).astype(np.float32))
    hists = []
    for s in range(3):
        edge = [0, 31, 32, V - 1]
        for w in range(1024, (V + 31) // 32, 1024):
            edge += [w * 32 - 1, w * 32, w * 32 + 31 if w * 32 + 31 < V else w * 32]
        hists.append(np.unique(np.concatenate([edge, r.integers(0, V, min(2000, V // 2))])))
    for row in range(6):                                     # zeros of both signs, seen and unseen
        h = hists[row % 3]
        unseen = np.setdiff1d(np.arange(V), h)
        x[row, h[1:5]] = [0.0, -0.0, 0.0, -0.0]
        x[row, unseen[:2]] = [0.0, -0.0]
    x[:, 0] = [3.5, -3.5, 0.0, -0.0, 1e-3, -250.0]           # column 0 and the last column: every sign
    x[:, V - 1] = [-7.25, 7.25, -0.0, 0.0, 300.0, -1e-3]
    return np_ops.bf16_round(x), hists                       # (the planted values too: both sides start from the same bf16 bits)


@pytest.mark.parametrize("V", [152064, 32064, 1003, 520])
def test_penalty_writeback_is_bit_exact(gpu, V):
    """`owc_penalize_rows_bf16` (penalize_rows_kernel, the kernel in front of every sampled draw under a repetition penalty) ==
    bf16_round(repetition_penalty_scores(x, ids, p)) as BITS: 4752 bitmap words (several per thread), 1002 words, a ragged last word
    (1003 % 32 = 11, % 8 = 3) and a small row; 6 rows over 3 bitmap rows through `row_slot` and 6 over 6 without; penalties above and
    below 1; set bits the kernel must ignore (at and above V, spare words).  Then the same launches with the rows at a stride > V (a
    multiple of 8 and an odd one) inside a canary buffer: nothing outside [row, 0 .. V) changes, the rows hold the same bits."""
    from lmms_owc_amd import ops

    x, hists = _writeback_case(V, V)
    row_slot = np.array([2, 0, 1, 0, 2, 1])
    seen3 = dev_bitmap(host_bitmap(hists, V), gpu)
    seen6 = dev_bitmap(host_bitmap([hists[s] for s in row_slot], V), gpu)
    for penalty in (1.05, 1.3, 0.7):
        want = bf16_t(np_ops.bf16_round(np.stack([Q.repetition_penalty_scores(x[i], hists[row_slot[i]], penalty) for i in range(6)]))).to(gpu)
        assert not torch.equal(want, bf16_t(x).to(gpu))
        got = ops.penalize_rows_bf16_(bf16_t(x).to(gpu), seen3, penalty, i32(row_slot, gpu))
        assert_same_bits(got, want, f"V={V} p={penalty} row_slot")
        got = ops.penalize_rows_bf16_(bf16_t(x).to(gpu), seen6, penalty)
        assert_same_bits(got, want, f"V={V} p={penalty} row_slot=None")
        # strided rows inside guard bands
        ld8 = (V + 8 + 256 + 15) // 16 * 16
        backing, inner = embed(bf16_t(x).to(gpu), CANARY[2], ld=ld8)
        assert inner.stride(0) % 8 == 0 and inner.stride(0) > V
        ops.penalize_rows_bf16_(inner, seen3, penalty, i32(row_slot, gpu))
        assert_guard_intact(backing, inner, f"V={V} p={penalty} ld={ld8}")
        assert_same_bits(inner, want, f"V={V} p={penalty} ld={ld8}")
        ld_odd = V + 37 + (V % 2)                              # odd, and > V
        assert ld_odd % 2 == 1
        backing, view = odd_strided(bf16_t(x).to(gpu), ld_odd, CANARY[2])
        expect = backing.clone()
        expect.as_strided((6, V), (ld_odd, 1), 300).copy_(want)
        ops.penalize_rows_bf16_(view, seen6, penalty)
        assert_same_bits(backing, expect, f"V={V} p={penalty} ld={ld_odd} (whole buffer, guard cells included)")


# ---- b. penalise, then sample, against the HF chain ---------------------------------------------------------------------------------
def _assert_counts(counts, probs, n, tag):
    """The suite's criterion (test_sampling_distribution_matches_the_hf_restatement): the support is the oracle's kept set, every
    token expected >= 20 times is within 5 sigma, and so is the pooled count of the rarer ones."""
    assert (counts[probs == 0] == 0).all(), f"{tag}: a token outside the kept set was drawn: {np.flatnonzero((counts > 0) & (probs == 0))[:8]}"
    exp = probs * n
    big = exp >= 20
    z = (counts[big] - exp[big]) / np.sqrt(exp[big] * (1 - probs[big]) + 1e-12)
    assert np.abs(z).max() < 5.0, (tag, float(np.abs(z).max()), int(big.sum()))
    assert abs(counts[~big].sum() - exp[~big].sum()) < 5.0 * np.sqrt(exp[~big].sum() + 1), tag


@pytest.mark.parametrize("V,R", [(1003, 60000), (152064, 4000)])
def test_penalise_then_sample_matches_the_hf_chain(gpu, V, R):
    """HF's chain for a sampled request under a repetition penalty (penalty -> temperature -> top-k -> top-p -> draw) through the two
    kernels the engine launches for it: R copies of one row, all penalised through ONE bitmap row, one random stream each.  Oracle:
    sampling_probs(bf16_round(penalised row)) - the write-back's rounding is part of the library's documented arithmetic (its cost
    is bounded in tests/test_oracle_sampling.py).  A missing penalty cannot pass: asserted on the host that it moves every kept set
    (no cut: the distribution, far beyond the 5 sigma the counts are held to)."""
    from lmms_owc_amd import ops

    row, hist, penalty = sampling_row(V)
    pen = np_ops.bf16_round(Q.repetition_penalty_scores(row, hist, penalty))
    seen = dev_bitmap(host_bitmap([hist], V), gpu)
    logits = bf16_t(row).to(gpu)[None].expand(R, V).contiguous()
    ops.penalize_rows_bf16_(logits, seen, penalty, torch.zeros(R, dtype=torch.int32, device=gpu))
    assert_same_bits(logits[R - 1:], bf16_t(pen)[None].to(gpu), f"V={V}: the last copy")
    for T, k, p in CONFIGS:
        probs, raw = S.sampling_probs(pen, T, k, p), S.sampling_probs(row, T, k, p)
        if k or p:
            assert not np.array_equal(probs > 0, raw > 0), "the penalty does not move the kept set: a missing penalty would pass"
        big = raw * R >= 20
        assert (np.abs(probs - raw)[big] * R / np.sqrt(raw[big] * R)).max() > 10, "the penalty moves no count by 10 sigma"
        got = to_np(ops.sample_bf16(logits, T, k, p, seed=4321)).astype(np.int64)
        _assert_counts(np.bincount(got, minlength=V), probs, R, f"V={V} T={T} k={k} p={p}")


# ---- c. the shipped configuration at op level ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [152064, 520])
def test_shipped_sampling_config_on_written_back_rows(gpu, V):
    """Qwen2-VL's generation_config.json at op level: `owc_sample_bf16` with top_k 1, top_p 0.001 on rows `owc_penalize_rows_bf16`
    wrote back returns the lowest-index argmax of the bf16 PENALISED values, exactly, at any temperature.  That is NOT always
    `owc_argmax_penalized_bf16`'s token (the argmax of the fp32 penalised scores, which is HF's single survivor): the count of rows
    where the two differ is asserted positive - the deviation that makes owc_llm_prefill / owc_llm_decode_step answer such a request
    through the penalised argmax (tests/test_qwen2vl_gpu.py) is real and visible here."""
    from lmms_owc_amd import ops

    x, hists = shipped_config_rows(V)
    penalty = 1.05
    f32 = np.stack([Q.repetition_penalty_scores(x[i], hists[i], penalty) for i in range(256)])
    a, b = np.argmax(f32, 1), np.argmax(np_ops.bf16_round(f32), 1)           # np.argmax: the lowest index among the maxima
    n_host = int((a != b).sum())
    assert n_host > 0, "the inputs show no deviation: pick others"
    seen = dev_bitmap(host_bitmap(hists, V), gpu)
    greedy = to_np(ops.argmax_penalized_bf16(bf16_t(x).to(gpu), seen, penalty)).astype(np.int64)
    assert np.array_equal(greedy, a)
    wb = ops.penalize_rows_bf16_(bf16_t(x).to(gpu), seen, penalty)
    for T in (0.01, 1.0):
        got = to_np(ops.sample_bf16(wb, T, 1, 0.001, seed=9)).astype(np.int64)
        assert np.array_equal(got, b), (V, T, np.flatnonzero(got != b)[:8])
        n = int((got != greedy).sum())
        print(f"[shipped-config] V={V} T={T}: {n} of 256 rows where the bf16 write-back changes the single survivor")
        assert n == n_host and n > 0


# ---- d. strides and guards for the other consumers -------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [152064, 1003, 520])
def test_logits_consumers_strided_inputs_and_guarded_outputs(gpu, V):
    """argmax, penalised argmax, sampler, beam candidates (plain and penalised), token log-probability: logits rows at a stride > V
    inside a NaN-poisoned buffer, every output inside canaries - the guard cells stay untouched and the results are bit-identical
    to the contiguous launch."""
    from lmms_owc_amd import ops

    r = np.random.default_rng(V + 1)
    rows, k, penalty = 5, 8, 1.3
    x = bf16_t(np_ops.bf16_round((r.standard_normal((rows, V)) * 3).astype(np.float32))).to(gpu)
    top = np.argsort(-to_np(x), axis=1, kind="stable")[:, :6]
    hists = [np.concatenate([top[i, ::2], [0, V - 1], r.integers(0, V, 50)]) for i in range(rows)]
    seen = dev_bitmap(host_bitmap(hists, V), gpu)
    target = i32([-1, 0, V - 1, int(top[3, 0]), int(r.integers(0, V))], gpu)
    p_back, xs = embed(x, POISON[2])
    p_before = p_back.clone()
    assert xs.stride(0) > V and xs.stride(0) % 8 == 0

    def outs(*shapes_dtypes):
        made = [guarded((int(np.prod(s)),), dt, gpu, CANARY[4]) for s, dt in shapes_dtypes]
        return made, [inner.view(s) for (_, inner), (s, _) in zip(made, shapes_dtypes)]

    def check(tag, made, got, want):
        for (backing, inner), g, w in zip(made, got, want):
            assert_guard_intact(backing, inner, f"V={V} {tag}")
            assert_same_bits(g, w, f"V={V} {tag}")

    I32, F32 = torch.int32, torch.float32
    # the two argmax kernels read 16-byte vectors (row stride % 8 == 0: a contiguous launch exists only where V % 8 == 0): held to numpy
    f = to_np(x)
    want_pen = [int(np.argmax(Q.repetition_penalty_scores(f[i], hists[i], penalty))) for i in range(rows)]
    assert want_pen != np.argmax(f, 1).tolist()               # (the penalty moves an argmax: half of each row's top tokens are seen)
    made, (o,) = outs(((rows,), I32))
    check("argmax", made, [ops.argmax_bf16(xs, out=o)], [i32(np.argmax(f, 1), gpu)])
    made, (o,) = outs(((rows,), I32))
    check("argmax_penalized", made, [ops.argmax_penalized_bf16(xs, seen, penalty, out=o)], [i32(want_pen, gpu)])
    if V % 8 == 0:
        assert_same_bits(ops.argmax_bf16(x), i32(np.argmax(f, 1), gpu), f"V={V} contiguous argmax")
        assert_same_bits(ops.argmax_penalized_bf16(x, seen, penalty), i32(want_pen, gpu), f"V={V} contiguous argmax_penalized")
    for T, tk, tp in ((0.9, 0, None), (0.7, 40, 0.8), (0.01, 1, 0.001)):
        made, (o,) = outs(((rows,), I32))
        check(f"sample T={T}", made, [ops.sample_bf16(xs, T, tk, tp, seed=3, out=o)], [ops.sample_bf16(x, T, tk, tp, seed=3)])
    made, o3 = outs(((rows,), F32), ((rows, k), F32), ((rows, k), I32))
    check("beam_candidates", made, ops.beam_candidates(xs, k, out=tuple(o3)), ops.beam_candidates(x, k))
    made, o3 = outs(((rows,), F32), ((rows, k), F32), ((rows, k), I32))
    check("beam_candidates_penalized", made, ops.beam_candidates_penalized(xs, k, seen, penalty, out=tuple(o3)),
          ops.beam_candidates_penalized(x, k, seen, penalty))
    made, (o,) = outs(((rows,), F32))
    check("token_logprob", made, [ops.token_logprob_bf16(xs, target, out=o)], [ops.token_logprob_bf16(x, target)])
    assert_same_bits(p_back, p_before, f"V={V}: the logits buffer (read-only for all of them)")


# ---- e. token_logprob_bf16 on its own ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [32064, 152064, 1003])
def test_token_logprob_vs_float64_log_softmax(gpu, V):
    """`owc_token_logprob_bf16` (LLaVA.loglikelihood's per-token term) against a float64 log-softmax of the same bf16 values: targets
    -1 (exactly 0), 0, V - 1, the row's argmax, random ids; one row shifted by +80 and one by -80 (the maximum must be subtracted
    before the exponential).  Bound: 2e-5 * max(1, max |want|), what test_beam_candidates_vs_numpy holds the same fp32 __expf /
    __logf summation to."""
    from lmms_owc_amd import ops

    r = np.random.default_rng(V + 7)
    x = (r.standard_normal((9, V)) * 3).astype(np.float32)
    x[4] += 80.0
    x[5] -= 80.0
    x = np_ops.bf16_round(x)
    target = r.integers(0, V, 9)
    target[:4] = [-1, 0, V - 1, int(np.argmax(x[3]))]
    target[8] = -1
    got = to_np(ops.token_logprob_bf16(bf16_t(x).to(gpu), i32(target, gpu)))
    f = x.astype(np.float64)
    m = f.max(1)
    logz = m + np.log(np.exp(f - m[:, None]).sum(1))
    want = np.where(target < 0, 0.0, f[np.arange(9), np.maximum(target, 0)] - logz)
    err = np.abs(got - want)
    print(f"[token-logprob] V={V}: max error {err.max():.3e} (bound {2e-5 * max(1.0, np.abs(want).max()):.3e})")
    assert (got[target < 0] == 0).all()
    assert err.max() <= 2e-5 * max(1.0, np.abs(want).max()), (err, want)
