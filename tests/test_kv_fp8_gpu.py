"""Op level of the fp8 (e4m3fn) KV cache: the prefill's row quantiser (owc_kv_quantize_fp8) and the fp8-cache form of the fused
decode attention (owc_decode_attention with kv_dtype = fp8).  The quantiser's arithmetic is owc_quantize_rows_fp8's, which
tests/test_fp8_gpu.py pins bit for bit on oracle/fp8_np.quantize_rows."""
import functools

import numpy as np
import pytest
import torch

from oracle import fp8_np as F
from oracle import qwen2vl_np as Q
from tests.util import bf16_randn, to_np

pytestmark = pytest.mark.gpu
HD = 128


def i32(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)


def quantize_cache(x):
    """bf16 [..., 128] -> (codes uint8 [..., 128], scales f32 [...]) by owc_quantize_rows_fp8."""
    from lmms_owc_amd import ops

    codes, scale = ops.quantize_rows_fp8(x.reshape(-1, HD).contiguous())
    return codes.view(x.shape), scale.view(x.shape[:-1])


@pytest.mark.parametrize("Hkv", [1, 4])
def test_kv_quantize_writes_exactly_the_rows_of_the_launch(gpu, Hkv):
    """40 token rows over 3 slots - 5 shared-prefix rows (tok_slot = -1) broadcast to slots [1, 3), an all-zero row, a row whose
    extremes are +-448 * scale: codes and scales equal owc_quantize_rows_fp8 of the staged rows, every other byte of the cache
    (codes and scales) is untouched."""
    from lmms_owc_amd import ops

    n_slots, s_max = 3, 24
    tok_slot = np.concatenate([np.full(5, -1), np.full(12, 0), np.full(11, 1), np.full(12, 2)])
    tok_idx = np.concatenate([np.arange(5), np.arange(12), np.arange(5, 16), np.arange(5, 17)])
    ks = bf16_randn((n_slots, Hkv, s_max, HD), 1, 1.0, gpu)
    vs = bf16_randn((n_slots, Hkv, s_max, HD), 2, 3.0, gpu)
    ks[2, :, :5], vs[2, :, :5] = ks[1, :, :5], vs[1, :, :5]      # a prefix row is staged alike in every slot of the broadcast
    ks[0, 0, 3] = 0                                              # zero row: scale 1, codes 0
    vs[1, 0, 7] = torch.linspace(-56, 56, HD, device=gpu).to(torch.bfloat16)   # amax = 448 * 2^-3: the ends saturate exactly at +-448
    g = torch.Generator(device=gpu).manual_seed(9)
    k8 = torch.randint(0, 256, ks.shape, generator=g, device=gpu, dtype=torch.uint8)
    v8 = torch.randint(0, 256, ks.shape, generator=g, device=gpu, dtype=torch.uint8)
    ksc = torch.rand(ks.shape[:-1], generator=g, device=gpu) + 7
    vsc = torch.rand(ks.shape[:-1], generator=g, device=gpu) + 7
    want = [k8.clone(), v8.clone(), ksc.clone(), vsc.clone()]
    (kq, kscale), (vq, vscale) = quantize_cache(ks), quantize_cache(vs)
    written = torch.zeros((n_slots, s_max), dtype=torch.bool, device=gpu)
    for sl, ix in zip(tok_slot, tok_idx):
        for s in ([1, 2] if sl < 0 else [sl]):
            written[s, ix] = True
    m = written[:, None, :].expand(n_slots, Hkv, s_max)
    for dst, src in zip(want, (kq, vq, kscale, vscale)):
        dst[m] = src[m]
    ops.kv_quantize_fp8_(ks, vs, k8, v8, ksc, vsc, i32(tok_slot, gpu), i32(tok_idx, gpu), Hkv, s_max, 1, 2)
    for got, w, name in zip((k8, v8, ksc, vsc), want, ("k codes", "v codes", "k scales", "v scales")):
        assert torch.equal(got, w), name
    assert int(written.sum()) == 12 + 16 + 17 and not m.all()
    assert ksc[0, 0, 3].item() == 1.0 and not k8[0, 0, 3].any()
    assert vsc[1, 0, 7].item() == 0.125 and v8[1, 0, 7, 0].item() == 0xFE and v8[1, 0, 7, -1].item() == 0x7E


KLEN = np.array([1, 63, 64, 65, 255, 256, 257, 300, 321, 336])   # tile (64) and four-wave-round (256) edges, a single key, s_max
S_MAX = 336


@functools.lru_cache(maxsize=None)
def decode_case(Hq, Hkv):
    """One fp8-cache decode step for a batch of len(KLEN) rows in permuted slots + the bf16-cache call on the same inputs."""
    from lmms_owc_amd import ops

    gpu = torch.device("cuda")
    B = len(KLEN)
    r = np.random.default_rng(Hq)
    slot = r.permutation(B + 2)[:B]
    pos = r.integers(0, 2000, B)
    qkv = bf16_randn((B, (Hq + 2 * Hkv) * HD), 4, 1.0, gpu)
    # rows of very different magnitude: the per-key scales matter
    mag = torch.from_numpy(np.exp2(r.uniform(-2, 2, (2, B + 2, Hkv, S_MAX, 1))).astype(np.float32)).to(gpu)
    kc0 = (bf16_randn((B + 2, Hkv, S_MAX, HD), 5, 1.0, gpu).float() * mag[0]).to(torch.bfloat16)
    vc0 = (bf16_randn((B + 2, Hkv, S_MAX, HD), 6, 1.0, gpu).float() * mag[1]).to(torch.bfloat16)
    cos, sin = ops.rope_table(2048, 64, 128, 1e6, True, gpu)
    dev = dict(pos=i32(pos, gpu), slot=i32(slot, gpu), widx=i32(KLEN - 1, gpu), klen=i32(KLEN, gpu))
    (k8, ksc), (v8, vsc) = quantize_cache(kc0), quantize_cache(vc0)
    before = [t.clone() for t in (k8, v8, ksc, vsc)]

    def run(rows=slice(None), nbuf1=None):
        from lmms_owc_amd import _lib

        cache = [t.clone() for t in before]
        lib = _lib.load()
        try:
            if nbuf1 is not None:
                assert lib.owc_tuning_set(b"decode_attn_nbuf1", nbuf1) == 0
            out = ops.decode_attention(qkv[rows], dev["pos"][rows], cos, sin, cache[0], cache[1], dev["slot"][rows], dev["widx"][rows],
                                       dev["klen"][rows], Hq, Hkv, S_MAX, HD ** -0.5, kv_dtype="fp8", k_scale=cache[2], v_scale=cache[3])
        finally:
            lib.owc_tuning_set(b"decode_attn_nbuf1", -1)
        return out, cache

    out, after = run()
    # the bf16-cache call: the K / V rows it writes are what the fp8 call must have quantised; mrope_kv gives the rotated q
    kc_b, vc_b = kc0.clone(), vc0.clone()
    ops.decode_attention(qkv, dev["pos"], cos, sin, kc_b, vc_b, dev["slot"], dev["widx"], dev["klen"], Hq, Hkv, S_MAX, HD ** -0.5)
    q_rot = qkv.clone()
    ops.mrope_kv_write_(q_rot, dev["pos"], cos, sin, kc0.clone(), vc0.clone(), dev["slot"], dev["widx"], Hq, Hkv, S_MAX, 16, 24, pos_stride=0)
    return dict(B=B, slot=slot, qkv=qkv, out=out, before=before, after=after, kc_b=kc_b, vc_b=vc_b, q_rot=q_rot, run=run)


SHAPES = [(2, 1), (28, 4), (64, 8), (16, 1)]


@pytest.mark.parametrize("Hq,Hkv", SHAPES)
def test_decode_step_writes_the_quantised_row_and_nothing_else(gpu, Hq, Hkv):
    """The fed token's row: codes and scale equal owc_quantize_rows_fp8 of the K (rotated) / V row the bf16-cache call writes for
    the same inputs; no other code or scale changes."""
    c = decode_case(Hq, Hkv)
    want = [t.clone() for t in c["before"]]
    (kq, ks), (vq, vs) = quantize_cache(c["kc_b"]), quantize_cache(c["vc_b"])
    for b in range(c["B"]):
        s, ix = int(c["slot"][b]), int(KLEN[b]) - 1
        want[0][s, :, ix], want[1][s, :, ix], want[2][s, :, ix], want[3][s, :, ix] = kq[s, :, ix], vq[s, :, ix], ks[s, :, ix], vs[s, :, ix]
    for got, w, name in zip(c["after"], want, ("k codes", "v codes", "k scales", "v scales")):
        assert torch.equal(got, w), name
    assert not torch.equal(c["after"][0], c["before"][0])


@pytest.mark.parametrize("Hq,Hkv", SHAPES)
def test_decode_attention_over_the_dequantised_cache(gpu, Hq, Hkv):
    """Against Q._attn (fp32) on codes * scale of the cache as the step left it - the fed token's row included, as the kernel reads
    it back.  Both sides see the same quantised K / V, so what remains is P's bf16 rounding and the summation order: the bound of the
    bf16 kernel family (tests/test_ops_gpu.py), 0.02 * max|want| + 1e-3."""
    c = decode_case(Hq, Hkv)
    G = Hq // Hkv
    k8, v8, ksc, vsc = (t.cpu().numpy() for t in c["after"])
    kd = F.e4m3_decode(k8) * ksc[..., None]
    vd = F.e4m3_decode(v8) * vsc[..., None]
    qn = to_np(c["q_rot"])[:, :Hq * HD].reshape(c["B"], Hq, HD)
    got = to_np(c["out"]).reshape(c["B"], Hq, HD)
    assert np.isfinite(got).all()
    for b in range(c["B"]):
        s, L = int(c["slot"][b]), int(KLEN[b])
        want = Q._attn(qn[b][:, None, :], np.repeat(kd[s, :, :L], G, 0), np.repeat(vd[s, :, :L], G, 0), HD ** -0.5, False, False)[:, 0]
        err = np.abs(got[b] - want).max()
        print(f"Hq {Hq} Hkv {Hkv} keys {L}: max err {err:.5f} of max|want| {np.abs(want).max():.4f}")
        assert err <= 0.02 * np.abs(want).max() + 1e-3, (b, L, err)


@pytest.mark.parametrize("Hq,Hkv", [(28, 4), (16, 1)])
def test_decode_forms_and_batches_give_the_same_bits(gpu, Hq, Hkv):
    """One V buffer per wave (large batches) against two (small batches): same bits, cache rows included; and a row's result does
    not depend on what else is in the batch."""
    c = decode_case(Hq, Hkv)
    out1, cache1 = c["run"](nbuf1=0)              # every launch takes the one-buffer form
    out2, cache2 = c["run"](nbuf1=1 << 30)        # every launch the two-buffer form
    assert torch.equal(out1, out2) and torch.equal(out1, c["out"])
    assert all(torch.equal(a, b) for a, b in zip(cache1, cache2))
    for b in (0, 7, c["B"] - 1):
        one, _ = c["run"](rows=slice(b, b + 1))
        assert torch.equal(one[0], c["out"][b]), b


def test_decode_attention_rejects_what_the_fp8_form_cannot_take(gpu):
    from lmms_owc_amd import _lib, ops

    c = decode_case(2, 1)
    k8, v8, ksc, vsc = c["before"]
    cos, sin = ops.rope_table(64, 64, 128, 1e6, True, gpu)
    z = i32([0], gpu)
    with pytest.raises(ValueError, match="kv_dtype"):
        ops.decode_attention(c["qkv"][:1], z, cos, sin, k8, v8, z, z, i32([1], gpu), 2, 1, S_MAX, 1.0, kv_dtype="int4")
    qkv = bf16_randn((1, (17 + 2) * HD), 1, 1.0, gpu)   # 17 query heads on one kv head: not a shape of the fused kernel
    with pytest.raises(_lib.OwcError):
        ops.decode_attention(qkv, z, cos, sin, k8, v8, z, z, i32([1], gpu), 17, 1, S_MAX, 1.0, kv_dtype="fp8", k_scale=ksc, v_scale=vsc)
