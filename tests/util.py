"""Helpers shared by the parity tests."""
import numpy as np
import torch


def to_np(t: torch.Tensor) -> np.ndarray:
    return t.detach().float().cpu().numpy()


def bf16_randn(shape, seed, scale=1.0, device="cpu"):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(torch.bfloat16).to(device)


def assert_bf16_close(got: np.ndarray, want: np.ndarray, ulps=2.0, min_exact=0.90, atol=1e-30):
    """Both sides are bf16-rounded values; accumulation order may move a result by a bf16 ulp."""
    got = got.astype(np.float32)
    want = want.astype(np.float32)
    assert got.shape == want.shape
    tol = ulps * np.maximum(np.abs(want), np.abs(got)) * 2.0**-8 + atol
    bad = np.abs(got - want) > tol
    assert not bad.any(), f"{bad.sum()} / {bad.size} beyond {ulps} bf16 ulp; max abs diff {np.abs(got - want).max()}"
    exact = (got == want).mean()
    assert exact >= min_exact, f"only {exact:.4f} bit-exact"


def check_forced_steps(got_logits, got_toks, ref_logits, ref_toks, frac, tag, mean_frac=None, margin_frac=None,
                       special_cols=None, special_frac=None) -> int:
    """Teacher-forced decode parity: EVERY step j of `got_logits` [T, V] is within `frac` * max |ref_logits[j]| of the
    reference's step-j logits (both conditional on the same forced continuation).  Token rule per step: where the
    reference's top-2 margin exceeds `margin_frac` (default 2 * the largest logit bound in force) * max|ref| the engine's argmax
    must equal the reference's (`ref_toks[j]`, or argmax(ref_logits[j]) when None); on a near-tie the engine's token must still
    score within that margin of the reference's maximum.  Never stops at a near-tie.  Returns the number of steps whose token
    was asserted equal.

    `special_cols` (vocabulary rows a test scaled up to create decisive margins, tests/test_decode_parity_gpu.py): the ordinary
    columns are then held to `frac` of THEIR OWN max |ref| (the statistic and bound of the unscaled case), the few scaled columns
    to `special_frac` of the global max |ref| (their error is the same hidden-state noise times the scale, over a handful of rows
    that also set the maximum: a heavier tail, observed up to 2.4 % where the ordinary columns sit at 1.0-1.5 %)."""
    got_logits, ref_logits = np.asarray(got_logits, np.float32), np.asarray(ref_logits, np.float32)
    assert got_logits.shape == ref_logits.shape, (got_logits.shape, ref_logits.shape)
    decisive, worst, worst_sp = 0, 0.0, 0.0
    main = np.ones(ref_logits.shape[1], bool)
    if special_cols is not None:
        main[np.asarray(special_cols)] = False
        assert special_frac is not None
    if margin_frac is None:
        margin_frac = 2 * (max(frac, special_frac) if special_cols is not None else frac)
    for j in range(ref_logits.shape[0]):
        ref, got = ref_logits[j], got_logits[j]
        scale = np.abs(ref).max()
        scale_main = np.abs(ref[main]).max()
        err = np.abs(got - ref)[main].max()
        worst = max(worst, float(err / scale_main))
        assert err <= frac * scale_main, f"{tag}: step {j} logits off by {err / scale_main:.4f} of max|logit| (bound {frac})"
        if special_cols is not None:
            err_sp = np.abs(got - ref)[~main].max()
            worst_sp = max(worst_sp, float(err_sp / scale))
            assert err_sp <= special_frac * scale, f"{tag}: step {j} scaled rows off by {err_sp / scale:.4f} of max|logit| (bound {special_frac})"
        if mean_frac is not None:
            assert np.abs(got - ref).mean() <= mean_frac * scale, f"{tag}: step {j} mean logit error"
        want = int(ref_toks[j]) if ref_toks is not None else int(np.argmax(ref))
        top2 = np.sort(ref)[-2:]
        if top2[1] - top2[0] > margin_frac * scale:
            assert int(got_toks[j]) == want, f"{tag}: step {j} token {int(got_toks[j])} != {want}"
            decisive += 1
        else:
            assert ref[int(got_toks[j])] >= top2[1] - margin_frac * scale, f"{tag}: step {j} picked a non-candidate token"
    sp = f", scaled rows {worst_sp:.4f} (bound {special_frac})" if special_cols is not None else ""
    print(f"[forced-steps] {tag}: {ref_logits.shape[0]} steps, worst logit error {worst:.4f} of max|logit| (bound {frac}){sp}, "
          f"{decisive} decisive token steps (margin > {margin_frac})")
    return decisive


def rel_step_errors(got_logits, ref_logits) -> np.ndarray:
    """Per step j: max |got[j] - ref[j]| / max |ref[j]|."""
    got, ref = np.asarray(got_logits, np.float32), np.asarray(ref_logits, np.float32)
    return np.array([np.abs(got[j] - ref[j]).max() / np.abs(ref[j]).max() for j in range(ref.shape[0])])


HF_NOISE_FACTOR = 1.5


def check_within_hf_bf16_noise(got_logits, hf_bf16_logits, hf_f32_logits, tag: str) -> None:
    """The HIP path computes in bf16 like HF's bf16 run, so its distance from HF's fp32 logits must be of the size of HF's OWN
    bf16-vs-fp32 gap (1.0-1.3 % of max |logit| on the committed goldens) - a regression that doubled the HIP error would still pass
    a fixed 2.5 % bound, it does not pass this one.  Asserted:
      * the worst step:  max_j err(HIP, f32)[j]  <= 1.5 x max_j err(HF-bf16, f32)[j];
      * the average:     mean_j err(HIP, f32)[j] <= 1.5 x mean_j err(HF-bf16, f32)[j];
      * per step:        err(HIP, f32)[j] <= 1.5 x err(HF-bf16, f32)[j] + 0.25 x (HF's worst step) - the additive term because two
        bf16 runs with different fp32 summation orders are two independent draws of the same noise: at a step where HF's
        draw happens to be small (0.55 % on one of these goldens) an equally good implementation is not bound to be small too."""
    e_hip, e_hf = rel_step_errors(got_logits, hf_f32_logits), rel_step_errors(hf_bf16_logits, hf_f32_logits)
    print(f"[hf-noise] {tag}: err(HIP, f32) {np.round(e_hip, 4).tolist()}  err(HF-bf16, f32) {np.round(e_hf, 4).tolist()}  "
          f"worst ratio {e_hip.max() / e_hf.max():.2f}  mean ratio {e_hip.mean() / e_hf.mean():.2f}  "
          f"per-step ratios {np.round(e_hip / e_hf, 2).tolist()}")
    assert e_hip.max() <= HF_NOISE_FACTOR * e_hf.max(), f"{tag}: worst step {e_hip.max():.4f} vs HF's own {e_hf.max():.4f}"
    assert e_hip.mean() <= HF_NOISE_FACTOR * e_hf.mean(), f"{tag}: mean over steps {e_hip.mean():.4f} vs HF's own {e_hf.mean():.4f}"
    lim = HF_NOISE_FACTOR * e_hf + 0.25 * e_hf.max()
    assert (e_hip <= lim).all(), f"{tag}: steps {np.flatnonzero(e_hip > lim).tolist()} beyond HF's bf16 noise: {e_hip} vs {e_hf}"


def assert_rel_close(got, ref, frac: float, tag: str = "") -> float:
    """max |got - ref| <= frac * max |ref|; prints the observed fraction so that the bounds can be kept at observed + headroom."""
    got, ref = np.asarray(got, np.float32), np.asarray(ref, np.float32)
    obs = float(np.abs(got - ref).max() / np.abs(ref).max())
    print(f"[rel-close] {tag}: {obs:.4f} of max|ref| (bound {frac})")
    assert obs <= frac, f"{tag}: off by {obs:.4f} of max|ref| (bound {frac})"
    return obs


# ---- guard bands and strided operands (tests/test_gemm_guard_gpu.py, tests/test_attention_guard_gpu.py, tests/test_ops_gpu.py) ----
# Bit patterns, by element size.  CANARY goes into OUTPUT buffers: a NaN with a payload that no kernel produces (f2bf of a NaN
# gives the quiet NaN 0x7FC0; the fp8 quantiser saturates and never emits the e4m3fn NaN 0xFF).  POISON goes into the padding
# of INPUT buffers: a NaN (quiet NaN for bf16 / f32, 0x7F for e4m3fn codes), so a read of padding that reaches an output shows.
_INT_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32}
CANARY = {1: 0xFF, 2: 0x7FA5, 4: 0x7FA5A5A5}
POISON = {1: 0x7F, 2: 0x7FC0, 4: 0x7FC00000}


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.view(_INT_VIEW[t.element_size()])


def _signed(pattern: int, item: int) -> int:
    """The bit pattern as a value of the integer view's dtype (uint8 for one byte, else signed)."""
    return pattern if item == 1 or pattern < (1 << (8 * item - 1)) else pattern - (1 << (8 * item))


def guarded(shape, dtype, device, fill, *, before=None, after=(256, 256), ld=None, size_ld=None):
    """A 2-D backing buffer filled with the bit pattern `fill` (CANARY / POISON above, indexed by element size) and the inner
    view of `shape` = (rows, cols) at row before[0], column before[1] of it: (backing, inner).

    before: default (1, 16 bytes) = (1, 8) for bf16 - the inner view's base address is then 16-byte aligned, which is all the
      C ABI promises, and (leading dimensions being multiples of 32 bytes here) not 32-byte aligned.
    after:  guard rows below and guard columns to the right of the inner view: at least the largest tile of any kernel under test
      (256 x 256), so that a whole unpredicated tile lands inside the allocation and fails an assert instead of faulting.
    ld:     leading dimension in elements (default: before[1] + cols + after[1], rounded up to 32 bytes); always a multiple of
      16 bytes, which satisfies every ABI rule (bf16 % 8, fp8 codes % 16 bytes, f32 % 4).
    size_ld: the largest leading dimension of ANY operand of the case: the backing gets as many elements as if its own rows had
      that pitch, so a kernel that uses another operand's leading dimension for this one still writes inside it.
    A 1-D `shape` (n,) gives a 1-D inner view (bias, scales) inside a one-row backing buffer."""
    one_d = len(shape) == 1
    rows, cols = (1, shape[0]) if one_d else shape
    item = torch.empty((), dtype=dtype).element_size()
    if before is None:
        before = (0 if one_d else 1, 16 // item)
    if one_d:
        after = (0, after[1])
    unit = 32 // item
    if ld is None:
        ld = -(-(before[1] + cols + after[1]) // unit) * unit
    assert ld >= before[1] + cols + after[1] and (ld * item) % 16 == 0, (ld, before, cols, after)
    n_rows = before[0] + rows + after[0]
    if size_ld is not None and size_ld > ld:
        n_rows = -(-n_rows * size_ld // ld)
    backing = torch.empty((n_rows, ld), dtype=dtype, device=device)
    _bits(backing).fill_(_signed(fill, item))
    inner = backing[before[0]:before[0] + rows, before[1]:before[1] + cols]
    assert inner.data_ptr() % 16 == 0
    return backing, (inner[0] if one_d else inner)


def embed(t: torch.Tensor, fill, **kw):
    """`t` (1-D or 2-D) copied into a `guarded` buffer of its own: (backing, inner view holding t's values)."""
    backing, inner = guarded(tuple(t.shape), t.dtype, t.device, fill, **kw)
    inner.copy_(t)
    return backing, inner


def assert_guard_intact(backing, inner, tag, fill=None, owned=None):
    """Every cell of `backing` outside the inner region still holds the fill pattern, compared AS INTEGERS.  `inner` is the view
    `guarded` returned; `owned` (optional bool tensor of inner's shape, or of backing's shape) narrows the region the kernel may
    write to the True cells (attention: the head_dim columns of the rows of each sequence).  Reports the first offending (row, column) pairs relative to
    the inner view (negative / beyond its shape = outside it)."""
    item = backing.element_size()
    fill = CANARY[item] if fill is None else fill
    ld = backing.stride(0)
    off = (inner.data_ptr() - backing.data_ptr()) // item
    r0, c0 = off // ld, off % ld
    rows, cols = (1, inner.shape[0]) if inner.dim() == 1 else inner.shape
    bits = _bits(backing)
    bad = bits != _signed(fill, item)
    if owned is None:
        bad[r0:r0 + rows, c0:c0 + cols] = False
    elif owned.shape == backing.shape:      # a mask over the whole backing buffer (layouts that are no rectangle of it)
        bad &= ~owned
    else:
        bad[r0:r0 + rows, c0:c0 + cols] &= ~owned.reshape(rows, cols)
    n_bad = int(bad.sum())
    if n_bad:
        where = torch.nonzero(bad)[:8].cpu().numpy()
        cells = [(int(r) - r0, int(c) - c0) for r, c in where]
        vals = [hex(int(bits[int(r), int(c)]) & ((1 << (8 * item)) - 1)) for r, c in where]
        raise AssertionError(f"{tag}: {n_bad} cells outside the owned region of the [{rows}, {cols}] view (ld {ld}) were written; first (row, col) "
                             f"relative to the view: {cells}, bits {vals}")


def assert_same_bits(got: torch.Tensor, want: torch.Tensor, tag: str) -> None:
    """Two tensors of the same shape and dtype hold the same bits (NaNs included); names the first differing cells."""
    assert got.shape == want.shape and got.dtype == want.dtype, (tag, got.shape, want.shape, got.dtype, want.dtype)
    diff = _bits(got.contiguous()) != _bits(want.contiguous())
    if bool(diff.any()):
        cells = [tuple(int(x) for x in c) for c in torch.nonzero(diff)[:8].cpu().numpy()]
        raise AssertionError(f"{tag}: {int(diff.sum())} / {diff.numel()} cells differ from the contiguous launch; first (row, col): {cells}")
