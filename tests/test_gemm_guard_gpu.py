"""Guard bands and strided operands for every GEMM kernel family (owc_gemm_bf16, owc_gemm_fp8, owc_gemm_f32).

tests/test_gemm_gpu.py, tests/test_fp8_gpu.py and tests/test_ops_gpu.py pin the ARITHMETIC of these kernels; every launch there has
lda == K, ldw == K, ldr == ldc == N, so a store past column N or row M lands in cells whose owner overwrites it (or in memory nobody
looks at), and a leading dimension used in place of another is the same number.  Here each case runs twice with the same knobs:

  (a) contiguous operands, as the existing tests launch it;
  (b) the same values embedded in larger buffers (tests/util.py `guarded`): A, W, R, bias (fp8: the scale vectors too) each with a
      DIFFERENT padding of NaNs, so lda, ldw, ldr, ldc all differ from the widths and from each other, and C inside a buffer of canaries
      (a NaN with a payload no kernel produces) with at least 256 guard rows and 256 guard columns - the largest tile - on the far
      sides.  Every backing buffer is sized for the largest leading dimension of the case, so a swapped pitch or a whole
      unpredicated tile writes wrong cells INSIDE the allocations: it fails an assert, it does not fault.

Asserted: (1) the canaries around C are intact, compared as integers; (2) C of (b) equals (a) bit for bit (strides change addresses,
not the K chain; the dispatch looks at M, N, K and bias != NULL only); (3) for the small shapes (a) agrees with the numpy oracle,
with the calls and tolerances of the existing tests of that epilogue.  The in-place residual (`residual` and `out` the same strided
view, as the models run it) takes its expected value from a copy made before the launch.

Families, the knobs that force each (restored afterwards to what the existing tests restore them to) and the shapes:

  bf16 (`launch()` in gemm_bf16.hip)
  | family                                | knobs                                                                | (M, N, K)                                         |
  | gemm_bf16_skinny_kernel, MT 1-4       | gemm_skinny_max_m 64                                                 | M in 1 / 17 / 33 / 64, N 272 (SwiGLU 288), K 256  |
  | gemm_bf16_skinny_kernel, 9-deep ring  | gemm_skinny_max_m 64                                                 | (5, 272, 8192)                                    |
  | gemm_bf16_nt_64_kernel 64x64          | gemm_small_tiles 2, gemm_skinny_max_m 0, gemm_mid_max_tiles 2^30     | (70, 264, 64 / 192 / 72 / 1024), gemm_k_pairs 0/1 |
  | gemm_bf16_nt_64_kernel 64x64, 3 stages| gemm_small_tiles 2, gemm_ring_128 0; gemm_small_tiles 3 (long K)     | (300, 7000, 64 / 72), (130, 3000, 1024)           |
  | gemm_bf16_nt_64_kernel 64x32, 32x32   | gemm_small_tiles 3 / 4, as above                                     | (70, 264, 64 / 192 / 1024), gemm_k_pairs 1 / 2    |
  | gemm_bf16_nt_64_kernel 128x64         | gemm_ring_128 1, gemm_mid_max_tiles 2^30                             | (513, 3600, 64), (513, 3208, 64 / 1024)           |
  | gemm_bf16_nt_64_kernel 32/64/128x160  | gemm_wide_tiles 1, gemm_skinny_max_m 0                               | M in 20 / 40 / 100, N 20352, K 128                |
  | gemm_bf16_nt_kernel 128x128           | gemm_mid_max_tiles 0, gemm_skinny_max_m 0                            | (130, 264, 64), (130, 264, 72: the K-tail form)   |
  | gemm_bf16_nt_256x128pp_kernel         | gemm_pp128 1, gemm_big_min_m 129                                     | (300, 392, 192)                                   |
  | gemm_bf16_nt_256_kernel (lock-step)   | gemm_pingpong 0, gemm_big_min_tiles 1                                | (500, 520, 192)                                   |
  | gemm_bf16_nt_256pp_kernel             | gemm_pingpong 1, gemm_big_min_tiles 1, gemm_nt_min_mb 0 / default,   | (500, 520, 128), (500, 520, 384)                  |
  |                                       | gemm_walk 0 / 2                                                      |                                                   |
  | gemm_bf16_nt_256pp_persist_kernel     | gemm_persist 1, gemm_nt_min_mb 0 / default                           | (4352, 4096, 384): 272 tiles                      |
  | short-last-round split (256pp+256x128)| gemm_tail_split 1                                                    | (512, 33024, 384)                                 |
  (SwiGLU needs N % 32 == 0: its cases use the next multiple of 32 - 288, 416, 544.)

  fp8 (`launch_fp8()` in gemm_fp8.hip; 128-byte K-tiles, K / 128 in 1, 2, 3 and - the long-K forms - 16)
  | gemm_fp8_skinny_kernel, MT 1-4        | gemm_skinny_max_m 64                                                 | M in 1 / 17 / 33 / 64, N 272 (288), K 384         |
  | gemm_fp8_nt_64_kernel 32/64/128x256   | default (M <= 128, 128-256 tile columns)                             | M in 20 / 40 / 100, N 32544, K 128 / 384          |
  | gemm_fp8_nt_64_kernel 32x32           | default                                                              | (70, 264, 128 / 256 / 384 / 2048)                 |
  | gemm_fp8_nt_64_kernel 64x32           | default                                                              | (300, 1000, 128 / 384 / 2048)                     |
  | gemm_fp8_nt_64_kernel 64x64           | default: SwiGLU; 257-512 blocks                                      | (70, 288, 128 / 256 / 384), (300, 3600, 384/2048) |
  | gemm_fp8_nt_64_kernel 128x64          | default                                                              | (513, 3600, 128 / 384)                            |
  | gemm_fp8_nt_256_kernel (lock-step)    | gemm_mid_max_tiles 0, gemm_pingpong 1                                | (500, 520, 128 / 384)                             |
  | gemm_fp8_nt_256pp_kernel              | gemm_mid_max_tiles 0, gemm_pingpong 2, gemm_nt_min_mb 0 / default    | (500, 520, 256 / 512)                             |

  f32 (`owc_gemm_f32`): (5, 64, 132), (257, 388, 384); none, gelu_erf, residual.

NOT covered, because no public entry point takes them with free leading dimensions: the rotary epilogue (OWC_EPI_VROPE, reached
only through owc_vit_forward) and the RMSNorm-fused GEMMs (gemm_bf16_skinny_norm_kernel and the NORMA form of
gemm_bf16_nt_64_kernel, reached only through owc_llm_decode_step); gemm_f32x3_nt_kernel runs only inside owc_bert_embed.
"""
import math
from contextlib import contextmanager

import numpy as np
import pytest
import torch

from oracle import fp8_np as F
from oracle import np_ops
from tests.util import CANARY, POISON, assert_bf16_close, assert_guard_intact, assert_same_bits, bf16_randn, embed, guarded, to_np

pytestmark = pytest.mark.gpu

# the value every knob goes back to (what tests/test_gemm_gpu.py / tests/test_fp8_gpu.py restore; the library's defaults otherwise)
RESTORE = {"gemm_skinny_max_m": -1, "gemm_mid_max_tiles": 256, "gemm_small_tiles": 1, "gemm_ring_128": -1, "gemm_wide_tiles": 1,
           "gemm_pp128": -1, "gemm_big_min_m": 129, "gemm_big_min_tiles": -1, "gemm_pingpong": -1, "gemm_nt_min_mb": -1, "gemm_walk": -1,
           "gemm_persist": -1, "gemm_tail_split": -1, "gemm_k_pairs": 1}
HUGE = 1 << 30


@contextmanager
def knobs(kv):
    from lmms_owc_amd import _lib

    lib = _lib.load()
    try:
        for name, value in kv.items():
            assert lib.owc_tuning_set(name.encode(), value) == 0, name
        yield
    finally:
        for name in kv:
            lib.owc_tuning_set(name.encode(), RESTORE[name])


def _lds(item, **cols):
    """One leading dimension per operand: 16 bytes of left guard + the width + 256 guard columns + a different extra padding each,
    rounded up to 32 bytes; returns (dict name -> ld, the largest).  `cols`: name = width, or name = (width, item size) for an
    operand whose elements are not `item` bytes (the fp32 C of OWC_EPILOGUE_F32)."""
    lds = {}
    for i, (name, c) in enumerate(cols.items()):
        c, it = c if isinstance(c, tuple) else (c, item)
        unit = 32 // it
        ld = -(-(16 // it + c + 256 + 48 * (i + 1)) // unit) * unit
        while ld in lds.values() or ld == c:
            ld += unit
        lds[name] = ld
    return lds, max(lds.values())


def _interleave(wg, wu):
    """gate / up rows interleaved in groups of 16: [g0..g15, u0..u15, g16.., u16..] (OWC_EPILOGUE_SWIGLU)."""
    f = wg.shape[0]
    return torch.stack([wg.reshape(f // 16, 16, -1), wu.reshape(f // 16, 16, -1)], dim=1).reshape(2 * f, -1).contiguous()


# ---------------------------------------------------------------------------------------------------------------- bf16
def _bf16_oracle(out, a, w, wg, wu, b, r, epi, large_kernel=False):
    """The calls and tolerances of tests/test_gemm_gpu.py for that epilogue: test_gemm_none, test_gemm_epilogues and - quick_gelu on the
    256-row tiles, `large_kernel` - test_gemm_epilogues_large_kernel."""
    if epi == "swiglu":
        g = np_ops.linear(to_np(a), to_np(wg), bf16=True)
        u = np_ops.linear(to_np(a), to_np(wu), bf16=True)
        want = np_ops.bf16_round(np_ops.silu(g, bf16=True) * u)
        assert_bf16_close(to_np(out), want, ulps=4.0, min_exact=0.80, atol=1e-4)
        return
    bn = None if b is None else to_np(b)
    if epi == "f32":
        np.testing.assert_allclose(to_np(out), np_ops.linear(to_np(a), to_np(w), bn), rtol=2e-5, atol=2e-4)
        return
    y = np_ops.linear(to_np(a), to_np(w), bn, bf16=True)
    if epi == "none":
        assert_bf16_close(to_np(out), y, atol=1e-4)
        return
    want = {"quick_gelu": lambda: np_ops.quick_gelu(y, bf16=True), "gelu_erf": lambda: np_ops.gelu_erf(y, bf16=True),
            "residual": lambda: np_ops.bf16_round(to_np(r) + y), "inplace": lambda: np_ops.bf16_round(to_np(r) + y)}[epi]()
    # a residual add can cancel: one bf16 ulp of the pre-add magnitude as absolute slack (test_gemm_epilogues)
    atol = 2.0 ** -7 * float(np.abs(y).max()) if epi in ("residual", "inplace") else 1e-4
    if large_kernel and epi == "quick_gelu":
        # test_gemm_epilogues_large_kernel: the activation maps a 1-ulp difference of its INPUT (accumulation order) to up to ~1.1 input
        # ulps of output, which is many output ulps where gelu(x) ~ 0: one input ulp of absolute slack
        atol = 2.0 ** -7 * float(np.abs(y).max())
    assert_bf16_close(to_np(out), want, ulps=4.0, min_exact=0.80, atol=atol)


def _bf16_case(gpu, m, n, k, epi, kv, oracle=True, bias=True, large_kernel=False):
    from lmms_owc_amd import _lib, ops

    E = {"none": _lib.EPI_NONE, "quick_gelu": _lib.EPI_QUICK_GELU, "gelu_erf": _lib.EPI_GELU_ERF, "residual": _lib.EPI_RESIDUAL,
         "inplace": _lib.EPI_RESIDUAL, "swiglu": _lib.EPI_SWIGLU, "f32": _lib.EPI_F32}[epi]
    if epi == "swiglu" and n % 32:
        n = -(-n // 32) * 32
    n_out = n // 2 if epi == "swiglu" else n
    tag = f"bf16 {epi} ({m}, {n}, {k}) {kv}"
    a = bf16_randn((m, k), 300 + m % 97, device=gpu)
    wg = wu = None
    if epi == "swiglu":
        wg = bf16_randn((n // 2, k), 308, 0.08, device=gpu)
        wu = bf16_randn((n // 2, k), 309, 0.08, device=gpu)
        w, b = _interleave(wg, wu), None
    else:
        w = bf16_randn((n, k), 305, 0.08, device=gpu)
        b = bf16_randn((n,), 306, device=gpu) if bias else None
    r = bf16_randn((m, n), 307, device=gpu) if epi in ("residual", "inplace") else None
    out_dtype = torch.float32 if epi == "f32" else torch.bfloat16
    item_c = 4 if epi == "f32" else 2
    lds, size_ld = _lds(2, a=k, w=k, r=n_out, c=(n_out, item_c))
    ldc = lds["c"]
    # size_ld goes to the INPUTS as well (a kernel that reads A or W with C's pitch then reads NaNs, not foreign memory): where W has
    # tens of thousands of rows - the wide and tail-split cases here, the fp8 wide cases below - its NaN-filled backing buffer is
    # 0.9-2.2 GB for the duration of the case
    _, ai = embed(a, POISON[2], ld=lds["a"], size_ld=size_ld)
    _, wi = embed(w, POISON[2], ld=lds["w"], size_ld=size_ld)
    bi = None if b is None else embed(b, POISON[2], after=(0, 256 + 32))[1]
    with knobs(kv):
        # (a) contiguous
        if epi == "inplace":
            want = r.clone()
            ops.gemm_bf16(a, w, b, epilogue=E, residual=want, out=want)
        else:
            want = ops.gemm_bf16(a, w, b, epilogue=E, residual=r)
        # (b) strided, guarded
        if epi == "inplace":
            cb, ci = embed(r, CANARY[2], ld=ldc, size_ld=size_ld)      # R and C: the same strided view inside canaries
            ops.gemm_bf16(ai, wi, bi, epilogue=E, residual=ci, out=ci)
        else:
            ri = None if r is None else embed(r, POISON[2], ld=lds["r"], size_ld=size_ld)[1]
            cb, ci = guarded((m, n_out), out_dtype, gpu, CANARY[item_c], ld=ldc, size_ld=size_ld)
            ops.gemm_bf16(ai, wi, bi, epilogue=E, residual=ri, out=ci)
        torch.cuda.synchronize()
    assert_guard_intact(cb, ci, tag)
    assert_same_bits(ci, want, tag)
    assert not bool(torch.isnan(ci).any()), f"{tag}: NaN in C (padding of an input was read)"
    if oracle:
        _bf16_oracle(want, a, w, wg, wu, b, r, epi, large_kernel)


RING = {"gemm_skinny_max_m": 0, "gemm_mid_max_tiles": HUGE}
BIG = {"gemm_big_min_tiles": 1}


def _bf16_cases():
    c = []

    def add(family, m, n, k, epi, kv, **kw):
        ident = f"{family}-{m}x{n}x{k}-{epi}" + "".join(f"-{a[5:]}{b}" for a, b in kv.items() if a in ("gemm_k_pairs", "gemm_nt_min_mb", "gemm_walk"))
        c.append(pytest.param(m, n, k, epi, kv, kw, id=ident))

    for m in (1, 17, 33, 64):
        for epi in ("none", "residual", "swiglu"):
            add("skinny", m, 272, 256, epi, {"gemm_skinny_max_m": 64})
    add("skinny9", 5, 272, 8192, "none", {"gemm_skinny_max_m": 64})
    for k in (64, 192, 72):
        for epi in ("none", "residual", "quick_gelu", "swiglu"):
            add("ring64x64", 70, 264, k, epi, {**RING, "gemm_small_tiles": 2})
    for kp in (0, 1):   # one K-tile per stage (16 K-tiles: the steady-state loop), two per stage
        for epi in ("none", "residual"):
            add("ring64x64", 70, 264, 1024, epi, {**RING, "gemm_small_tiles": 2, "gemm_k_pairs": kp})
    for name, st in (("ring64x32", 3), ("ring32x32", 4)):
        for epi in ("none", "residual"):
            for k in (64, 192):
                add(name, 70, 264, k, epi, {**RING, "gemm_small_tiles": st})
            for kp in (1, 2):   # four / two K-tiles per stage
                add(name, 70, 264, 1024, epi, {**RING, "gemm_small_tiles": st, "gemm_k_pairs": kp})
    for k in (64, 72):      # 550 blocks of 64x64 (513-768): the three-stage form, with and without the K tail
        for epi in ("none", "residual"):
            add("ring64x64s3", 300, 7000, k, epi, {**RING, "gemm_small_tiles": 2, "gemm_ring_128": 0})
    for epi in ("none", "residual"):   # 64x32 forced, long K, 282 blocks (two rounds) but 141 of 64x64: three stages of 64x64, two K-tiles each
        add("ring64x64s3k2", 130, 3000, 1024, epi, {**RING, "gemm_small_tiles": 3})
    for epi in ("none", "residual"):
        add("ring128x64", 513, 3600, 64, epi, {"gemm_ring_128": 1, "gemm_mid_max_tiles": HUGE})      # 285 blocks: three stages, two per CU
    add("ring128x64", 513, 3208, 64, "none", {"gemm_ring_128": 1, "gemm_mid_max_tiles": HUGE})       # 255 blocks: four stages
    add("ring128x64", 513, 3208, 1024, "residual", {"gemm_ring_128": 1, "gemm_mid_max_tiles": HUGE})  # two K-tiles per stage
    for m in (20, 40, 100):
        for epi in ("none", "swiglu"):
            add("wide160", m, 20352, 128, epi, {"gemm_wide_tiles": 1, "gemm_skinny_max_m": 0})
    for k in (64, 72):
        for epi in ("none", "quick_gelu", "gelu_erf", "residual", "swiglu", "f32"):
            add("128x128", 130, 264, k, epi, {"gemm_mid_max_tiles": 0, "gemm_skinny_max_m": 0})
    for epi in ("none", "residual", "quick_gelu", "swiglu"):
        add("256x128pp", 300, 392, 192, epi, {"gemm_pp128": 1, "gemm_big_min_m": 129}, large_kernel=True)
    for epi in ("none", "residual", "gelu_erf", "swiglu", "f32"):
        add("256lockstep", 500, 520, 192, epi, {**BIG, "gemm_pingpong": 0}, large_kernel=True)
    for k in (128, 384):
        for nt in (0, -1):
            for walk in (0, 2):
                for epi in ("none", "residual", "quick_gelu", "swiglu", "f32"):
                    add("256pp", 500, 520, k, epi, {**BIG, "gemm_pingpong": 1, "gemm_nt_min_mb": nt, "gemm_walk": walk}, large_kernel=True)
    for nt in (0, -1):
        for epi in ("none", "inplace", "gelu_erf"):
            add("persist", 4352, 4096, 384, epi, {"gemm_persist": 1, "gemm_nt_min_mb": nt}, oracle=False)
    for epi in ("none", "swiglu"):
        add("tailsplit", 512, 33024, 384, epi, {"gemm_tail_split": 1}, oracle=False, bias=False)
    return c


@pytest.mark.parametrize("m,n,k,epi,kv,kw", _bf16_cases())
def test_gemm_bf16_guard_and_strides(gpu, m, n, k, epi, kv, kw):
    _bf16_case(gpu, m, n, k, epi, kv, **kw)


# ----------------------------------------------------------------------------------------------------------------- fp8
def _fp8_case(gpu, m, n, k, epi, kv):
    from lmms_owc_amd import _lib, ops

    E = {"bias": _lib.EPI_NONE, "res": _lib.EPI_RESIDUAL, "swiglu": _lib.EPI_SWIGLU}[epi]
    if epi == "swiglu" and n % 32:
        n = -(-n // 32) * 32
    n_out = n // 2 if epi == "swiglu" else n
    tag = f"fp8 {epi} ({m}, {n}, {k}) {kv}"
    x = bf16_randn((m, k), 380 + m % 97, 1.0, gpu)
    w = bf16_randn((n, k), 381, 0.05, gpu)
    xq, xs = ops.quantize_rows_fp8(x)
    wq, ws = ops.quantize_rows_fp8(w)
    nxq, nxs, nwq, nws = xq.cpu().numpy(), to_np(xs), wq.cpu().numpy(), to_np(ws)
    bias = bf16_randn((n,), 5, 0.5, gpu) if epi == "bias" else None
    r = bf16_randn((m, n), 9, 1.0, gpu) if epi == "res" else None
    if epi == "swiglu":   # rows [0, f) = gate, [f, 2f) = up for the oracle; interleaved per 16 (codes and scales alike) for the kernel
        f = n // 2
        kq, ks = _interleave(wq[:f], wq[f:]), _interleave(ws[:f, None], ws[f:, None])[:, 0].contiguous()
    else:
        kq, ks = wq, ws
    lds8, _ = _lds(1, a=k, w=k)
    lds16, _ = _lds(2, r=n_out, c=n_out)
    size_ld = max(max(lds8.values()), 2 * max(lds16.values()))     # whichever pitch, in bytes or in elements, is used for whichever operand
    _, ai = embed(xq, POISON[1], ld=lds8["a"], size_ld=size_ld)
    _, wi = embed(kq, POISON[1], ld=lds8["w"], size_ld=size_ld)
    _, sai = embed(xs, POISON[4], after=(0, 256))
    _, swi = embed(ks, POISON[4], after=(0, 256 + 40))
    bi = None if bias is None else embed(bias, POISON[2], after=(0, 256 + 32))[1]
    ri = None if r is None else embed(r, POISON[2], ld=lds16["r"], size_ld=size_ld)[1]
    cb, ci = guarded((m, n_out), torch.bfloat16, gpu, CANARY[2], ld=lds16["c"], size_ld=size_ld)
    with knobs(kv):
        want_t = ops.gemm_fp8(xq, xs, kq, ks, bias, epilogue=E, residual=r)
        ops.gemm_fp8(ai, sai, wi, swi, bi, epilogue=E, residual=ri, out=ci)
        torch.cuda.synchronize()
    assert_guard_intact(cb, ci, tag)
    assert_same_bits(ci, want_t, tag)
    assert not bool(torch.isnan(ci).any()), f"{tag}: NaN in C (padding of an input was read)"
    # oracle: tests/test_fp8_gpu.py::test_gemm_fp8_matches_oracle
    out = to_np(want_t)
    if epi == "swiglu":
        y = F.linear_fp8(None, nwq, nws, xq=nxq, xs=nxs)
        g, u = y[:, :f], y[:, f:]
        want = np_ops.bf16_round(np_ops.bf16_round(g / (1.0 + np.exp(-g))) * u)
        assert np.abs(out - want).max() <= 2.0 ** -6 * np.abs(want).max()
    elif epi == "res":
        want = np_ops.bf16_round(F.linear_fp8(None, nwq, nws, xq=nxq, xs=nxs) + to_np(r))
        assert np.abs(out - want).max() <= 2.0 ** -7 * np.abs(want).max()
    else:
        want = F.linear_fp8(None, nwq, nws, to_np(bias), xq=nxq, xs=nxs)
        assert_bf16_close(out, want, ulps=2.0, min_exact=0.95, atol=2.0 ** -9 * np.abs(want).max())


def _fp8_cases():
    c = []

    def add(family, m, n, k, epi, kv=None):
        kv = kv or {}
        ident = f"{family}-{m}x{n}x{k}-{epi}" + ("-nt0" if kv.get("gemm_nt_min_mb") == 0 else "")
        c.append(pytest.param(m, n, k, epi, kv, id=ident))

    for m in (1, 17, 33, 64):
        for epi in ("bias", "res", "swiglu"):
            add("skinny", m, 272, 384, epi, {"gemm_skinny_max_m": 64})
    for k in (128, 256):
        add("skinny", 17, 272, k, "bias", {"gemm_skinny_max_m": 64})
    for m in (20, 40, 100):
        for epi in ("bias", "swiglu"):
            add("wide256", m, 32544, 128, epi)
    add("wide256", 40, 32544, 384, "bias")
    for k in (128, 256, 384, 2048):
        for epi in ("bias", "res"):
            add("ring32x32", 70, 264, k, epi)
    for k in (128, 384, 2048):
        for epi in ("bias", "res"):
            add("ring64x32", 300, 1000, k, epi)
    for k in (128, 256, 384):
        add("ring64x64", 70, 288, k, "swiglu")
    for k in (384, 2048):     # 285 blocks of 64x64: one K-tile per stage, and (K >= 2048) two
        for epi in ("bias", "res"):
            add("ring64x64", 300, 3600, k, epi)
    for k in (128, 384):
        for epi in ("bias", "res"):
            add("ring128x64", 513, 3600, k, epi)
    for k in (128, 384):
        for epi in ("bias", "res", "swiglu"):
            add("256lockstep", 500, 520, k, epi, {"gemm_skinny_max_m": 0, "gemm_mid_max_tiles": 0, "gemm_pingpong": 1})
    for k in (256, 512):
        for nt in (0, -1):
            for epi in ("bias", "res", "swiglu"):
                add("256pp", 500, 520, k, epi, {"gemm_skinny_max_m": 0, "gemm_mid_max_tiles": 0, "gemm_pingpong": 2, "gemm_nt_min_mb": nt})
    return c


@pytest.mark.parametrize("m,n,k,epi,kv", _fp8_cases())
def test_gemm_fp8_guard_and_strides(gpu, m, n, k, epi, kv):
    _fp8_case(gpu, m, n, k, epi, kv)


# ----------------------------------------------------------------------------------------------------------------- f32
@pytest.mark.parametrize("epi", ["none", "gelu", "res"])
@pytest.mark.parametrize("m,n,k", [(5, 64, 132), (257, 388, 384)])
def test_gemm_f32_guard_and_strides(gpu, m, n, k, epi):
    from lmms_owc_amd import _lib, ops

    tag = f"f32 {epi} ({m}, {n}, {k})"
    g = torch.Generator().manual_seed(1)
    a = torch.randn(m, k, generator=g).to(gpu)
    w = (torch.randn(n, k, generator=g) / math.sqrt(k)).to(gpu)
    b = torch.randn(n, generator=g).to(gpu)
    r = torch.randn(m, n, generator=g).to(gpu) if epi == "res" else None
    E = {"none": _lib.EPI_NONE, "gelu": _lib.EPI_GELU_ERF, "res": _lib.EPI_RESIDUAL}[epi]
    lds, size_ld = _lds(4, a=k, w=k, r=n, c=n)
    _, ai = embed(a, POISON[4], ld=lds["a"], size_ld=size_ld)
    _, wi = embed(w, POISON[4], ld=lds["w"], size_ld=size_ld)
    _, bi = embed(b, POISON[4], after=(0, 256 + 24))
    ri = None if r is None else embed(r, POISON[4], ld=lds["r"], size_ld=size_ld)[1]
    cb, ci = guarded((m, n), torch.float32, gpu, CANARY[4], ld=lds["c"], size_ld=size_ld)
    want_t = ops.gemm_f32(a, w, b, epilogue=E, residual=r)
    ops.gemm_f32(ai, wi, bi, epilogue=E, residual=ri, out=ci)
    torch.cuda.synchronize()
    assert_guard_intact(cb, ci, tag)
    assert_same_bits(ci, want_t, tag)
    assert not bool(torch.isnan(ci).any()), f"{tag}: NaN in C (padding of an input was read)"
    # oracle and tolerance: tests/test_ops_gpu.py::test_gemm_f32
    y = to_np(a).astype(np.float64) @ to_np(w).astype(np.float64).T + to_np(b)
    want = np_ops.gelu_erf(y.astype(np.float32)) if epi == "gelu" else (y + to_np(r) if epi == "res" else y)
    np.testing.assert_allclose(to_np(want_t), want, rtol=1e-5, atol=2e-5)
