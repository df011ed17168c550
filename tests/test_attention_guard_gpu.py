"""Guard bands and strided operands for the attention kernels (owc_attention_bf16, owc_decode_attention).

tests/test_attention_accuracy_gpu.py and tests/test_ops_gpu.py hold these kernels to a float64 / fp32 softmax, always with the
sequences and heads packed back to back: a store past head_dim (columns 80-95 of the head_dim-80 tile) lands in the next head, a
store past a sequence's last row in the next sequence, and the rightful owner overwrites both; q_ts / k_ts / v_ts / o_ts and the
head strides are tied to each other.  Here every kernel runs twice with the same knobs - packed, as the existing tests launch it,
and in a layout none of them uses:

  * O: o_hs > head_dim (guard columns between heads), o_ts > n_heads * o_hs, the sequences placed through o_start with gaps of at
    least 128 canary rows (the query block) between them and 256 rows after the last one; o_ts % 4 == 0, o_hs % 4 == 0 - the ABI's rule;
  * Q, K, V: slices of NaN-filled buffers, each with strides of its own (and K / V rows that start elsewhere than the Q rows), and
    the fused [T, 3, H, head_dim] layout with padding after each head and after each row;
  * lengths that leave partial query blocks and partial key tiles: [1, 63, 65, 129] for the vision kernels, [7, 130, 257] causal
    (also behind a 15-key shared prefix: q_len < seq_len), key counts [1, 64, 65, 257] for the decode mapping and the fused decode step.

Asserted: every cell of the O buffer outside the owned ones still holds the canary (compared as integers; the message names the
first offending (row, column) pairs); the owned cells equal the packed launch bit for bit; no NaN among them (a read of padding
that reaches an output).

Kernels: attn_fwd_kernel<80 / 64, non-causal> (attn_mfma32 0), attn_fwd32_kernel / attn_fwd32p_kernel<80 / 64> (attn_mfma32 1 / 2),
attn_fwd_kernel<128, causal> with attn_gqa_pack 0 / 1, attn_fwd_kernel<128, non-causal> in the decode mapping (q_len = the heads of a
kv group), attn_decode_fused_kernel<NBUF 1 / 2, bf16 / fp8 cache> (decode_attn_nbuf1 0 / huge).  head_dim 32 is not launched by any
model fixture of the suite (the sentence encoder has its own attention kernel in bert.hip), so it has no case here.
"""
import numpy as np
import pytest
import torch

from tests.util import CANARY, POISON, assert_guard_intact, assert_same_bits, bf16_randn, embed, guarded

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


def _i32(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)


def _flat_index(lens, starts, H, hd, ts, hs, dev):
    """Element offsets of (sequence b, row i, head h, dim d) = (starts[b] + i) * ts + h * hs + d, as an int64 tensor [sum(lens), H, hd]
    in the order of a packed [T, H, hd] tensor."""
    rows = torch.cat([torch.arange(n, dtype=torch.int64) + int(s) for n, s in zip(lens, starts)])
    idx = rows[:, None, None] * ts + torch.arange(H, dtype=torch.int64)[None, :, None] * hs + torch.arange(hd, dtype=torch.int64)[None, None, :]
    return idx.to(dev)


def _filled(n, pattern, dev):
    buf = torch.empty(n, dtype=BF16, device=dev)
    buf.view(torch.int16).fill_(pattern)
    return buf


def _place(vals, idx, ts, dev, base=None):
    """A NaN-filled flat bf16 buffer with `vals` [T, H, hd] at offsets base + idx; (buffer, the view the kernel gets).  base: one row
    + 16 bytes, so the kernel's pointer is 16-byte aligned and no more than the ABI promises; 64 rows of NaN follow the last element."""
    base = ts + 8 if base is None else base
    buf = _filled(base + int(idx.max()) + 1 + 64 * ts, POISON[2], dev)
    buf[base + idx.reshape(-1)] = vals.reshape(-1)
    return buf, buf[base:]


class _Out:
    """The O buffer of one strided launch: canaries everywhere, 2-D [rows, o_ts] so that an offending cell is reported as
    (token row, column) relative to the kernel's O pointer; 256 canary rows follow the last owned row."""

    def __init__(self, idx, o_ts, dev):
        self.idx, self.o_ts = idx, o_ts
        self.base = 2 * o_ts + 8                 # (o_ts % 4 == 0: 16-byte aligned)
        n_rows = 2 + (int(idx.max()) // o_ts + 1) + 256 + 1
        self.backing = _filled(n_rows * o_ts, CANARY[2], dev).view(n_rows, o_ts)
        self.ptr = self.backing.view(-1)[self.base:]

    def check(self, want, tag):
        """want: the packed launch's output in the order of idx ([T, H, hd])."""
        owned = torch.zeros(self.backing.shape, dtype=torch.bool, device=self.backing.device)
        owned.view(-1)[self.base + self.idx.reshape(-1)] = True
        assert_guard_intact(self.backing, self.backing[2:, 8:], tag, owned=owned)
        got = self.ptr[self.idx.reshape(-1)].reshape(want.shape)
        assert_same_bits(got, want, tag)
        assert not bool(torch.isnan(got).any()), f"{tag}: NaN in O (padding of an input was read)"


def _gapped(lens, gap):
    """start rows with `gap` foreign rows in front of every sequence."""
    out, at = [], 0
    for n in lens:
        at += gap
        out.append(at)
        at += n
    return np.asarray(out)


VISION_LENS = [1, 63, 65, 129]


@pytest.mark.parametrize("layout", ["separate", "fused"])
@pytest.mark.parametrize("mfma32", [0, 1, 2])
@pytest.mark.parametrize("hd", [80, 64])
def test_vision_attention_guard_and_strides(gpu, hd, mfma32, layout):
    from lmms_owc_amd import _lib, ops

    lib = _lib.load()
    H, lens = 3, VISION_LENS
    T, n = sum(lens), len(lens)
    tag = f"vision attention hd{hd} attn_mfma32={mfma32} {layout}"
    qkv = bf16_randn((T, 3, H, hd), 400 + hd, 1.3, gpu)
    E = H * hd
    packed = qkv.reshape(T, 3 * E)
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
    kw = dict(n_seq=n, n_heads=H, kv_group=1, head_dim=hd, max_q_len=max(lens), causal=False, scale=hd ** -0.5)
    o_hs = hd + 20
    o_ts = H * o_hs + 24
    out = _Out(_flat_index(lens, _gapped(lens, 130), H, hd, o_ts, o_hs, gpu), o_ts, gpu)
    o_start = _i32(_gapped(lens, 130), gpu)
    try:
        assert lib.owc_tuning_set(b"attn_mfma32", mfma32) == 0
        want = torch.zeros((T, E), dtype=BF16, device=gpu)
        ops.attention(packed, 3 * E, hd, packed[:, E:], 3 * E, hd, packed[:, 2 * E:], 3 * E, hd, want, E, hd, _i32(starts, gpu),
                      _i32(starts, gpu), _i32(lens, gpu), **kw)
        if layout == "fused":      # one [rows, 3, H, hs] buffer: padding after each head and after each row, NaN rows between the sequences
            hs = hd + 24
            ts = 3 * H * hs + 40
            st = _gapped(lens, 3)
            idx = _flat_index(lens, st, H, hd, ts, hs, gpu)
            base = ts + 8
            buf = _filled(base + int(idx.max()) + 2 * H * hs + 1 + 64 * ts, POISON[2], gpu)
            for j in range(3):
                buf[base + j * H * hs + idx.reshape(-1)] = qkv[:, j].reshape(-1)
            q, k, v = buf[base:], buf[base + H * hs:], buf[base + 2 * H * hs:]
            ops.attention(q, ts, hs, k, ts, hs, v, ts, hs, out.ptr, o_ts, o_hs, _i32(st, gpu), _i32(st, gpu), _i32(lens, gpu), o_start=o_start, **kw)
        else:                      # three buffers, three pairs of strides, K / V rows that start elsewhere than the Q rows
            (q_hs, q_ts), (k_hs, k_ts), (v_hs, v_ts) = (hd + 8, H * (hd + 8) + 16), (hd + 16, H * (hd + 16) + 8), (hd + 40, H * (hd + 40) + 24)
            q_st, k_st = _gapped(lens, 2), _gapped(lens, 5)
            _, q = _place(qkv[:, 0], _flat_index(lens, q_st, H, hd, q_ts, q_hs, gpu), q_ts, gpu)
            _, k = _place(qkv[:, 1], _flat_index(lens, k_st, H, hd, k_ts, k_hs, gpu), k_ts, gpu)
            _, v = _place(qkv[:, 2], _flat_index(lens, k_st, H, hd, v_ts, v_hs, gpu), v_ts, gpu)
            ops.attention(q, q_ts, q_hs, k, k_ts, k_hs, v, v_ts, v_hs, out.ptr, o_ts, o_hs, _i32(q_st, gpu), _i32(k_st, gpu), _i32(lens, gpu),
                          o_start=o_start, **kw)
        torch.cuda.synchronize()
    finally:
        lib.owc_tuning_set(b"attn_mfma32", -1)
    out.check(want.reshape(T, H, hd), tag)


def _cache_layout(n, Hkv, s_max, ts):
    """K / V rows of n sequences x Hkv heads x s_max keys with row pitch ts > hd, head stride hs > s_max * ts and NaN rows between the
    sequences: (hs, k_start [n] in rows of ts)."""
    hs = s_max * ts + 24
    per_seq = -(-Hkv * hs // ts) + 3
    return hs, 2 + np.arange(n) * per_seq


@pytest.mark.parametrize("prefix", [0, 15])
@pytest.mark.parametrize("pack", [0, 1])
def test_causal_attention_guard_and_strides(gpu, pack, prefix):
    from lmms_owc_amd import _lib, ops

    lib = _lib.load()
    Hq, Hkv, hd, s_max, lens = 4, 2, 128, 280, [7, 130, 257]
    n, T = len(lens), sum(lens)
    klen = [x + prefix for x in lens]
    tag = f"causal attention attn_gqa_pack={pack} prefix={prefix}"
    q = bf16_randn((T, Hq, hd), 411, 1.0, gpu)
    kc = bf16_randn((n, Hkv, s_max, hd), 412, 1.0, gpu)
    vc = bf16_randn((n, Hkv, s_max, hd), 413, 1.0, gpu)
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
    kw = dict(n_seq=n, n_heads=Hq, kv_group=Hq // Hkv, head_dim=hd, max_q_len=max(lens), causal=True, scale=hd ** -0.5,
              q_len=_i32(lens, gpu) if prefix else None)
    o_hs = hd + 12
    o_ts = Hq * o_hs + 20
    o_st = _gapped(lens, 130)
    out = _Out(_flat_index(lens, o_st, Hq, hd, o_ts, o_hs, gpu), o_ts, gpu)
    q_hs = hd + 8
    q_ts = Hq * q_hs + 16
    q_st = _gapped(lens, 2)
    _, qs = _place(q, _flat_index(lens, q_st, Hq, hd, q_ts, q_hs, gpu), q_ts, gpu)
    # only the keys a sequence owns are placed: everything else in the K / V buffers (keys beyond its length included) is NaN
    keys = torch.cat([kc[b, :, :klen[b]].transpose(0, 1) for b in range(n)])     # [sum(klen), Hkv, hd]
    vals = torch.cat([vc[b, :, :klen[b]].transpose(0, 1) for b in range(n)])
    k_ts, v_ts = hd + 8, hd + 24
    k_hs, k_st = _cache_layout(n, Hkv, s_max, k_ts)
    v_hs = s_max * v_ts + 40
    assert Hkv * v_hs <= (k_st[1] - k_st[0]) * v_ts       # V shares k_start: its sequences do not overlap either
    _, ks = _place(keys, _flat_index(klen, k_st, Hkv, hd, k_ts, k_hs, gpu), k_ts, gpu)
    _, vs = _place(vals, _flat_index(klen, k_st, Hkv, hd, v_ts, v_hs, gpu), v_ts, gpu)
    try:
        assert lib.owc_tuning_set(b"attn_gqa_pack", pack) == 0
        want = torch.zeros((T, Hq * hd), dtype=BF16, device=gpu)
        ops.attention(q.reshape(T, Hq * hd), Hq * hd, hd, kc, hd, s_max * hd, vc, hd, s_max * hd, want, Hq * hd, hd, _i32(starts, gpu),
                      _i32(np.arange(n) * Hkv * s_max, gpu), _i32(klen, gpu), **kw)
        ops.attention(qs, q_ts, q_hs, ks, k_ts, k_hs, vs, v_ts, v_hs, out.ptr, o_ts, o_hs, _i32(q_st, gpu), _i32(k_st, gpu), _i32(klen, gpu),
                      o_start=_i32(o_st, gpu), **kw)
        torch.cuda.synchronize()
    finally:
        lib.owc_tuning_set(b"attn_gqa_pack", 1)
    out.check(want.reshape(T, Hq, hd), tag)


DECODE_KLEN = [1, 64, 65, 257]


def test_decode_mapping_attention_guard_and_strides(gpu):
    """The decode-step mapping of owc_attention_bf16 (tests/test_ops_gpu.py::test_attention_decode_mapping): the G query heads of a kv
    group are the `q_len` rows of a (sequence, kv head) pair."""
    from lmms_owc_amd import ops

    Hq, Hkv, hd, s_max = 12, 2, 128, 264
    G, klen = Hq // Hkv, DECODE_KLEN
    B = len(klen)
    tag = "decode mapping of owc_attention_bf16"
    qkv = bf16_randn((B, (Hq + 2 * Hkv) * hd), 421, 1.0, gpu)
    kc = bf16_randn((B, Hkv, s_max, hd), 422, 1.0, gpu)
    vc = bf16_randn((B, Hkv, s_max, hd), 423, 1.0, gpu)
    ar = np.arange(B)
    kw = dict(n_seq=B, n_heads=Hkv, kv_group=1, head_dim=hd, max_q_len=G, causal=False, scale=hd ** -0.5, q_len=_i32(np.full(B, G), gpu))
    want = torch.zeros((B, Hq * hd), dtype=BF16, device=gpu)
    ops.attention(qkv, hd, G * hd, kc, hd, s_max * hd, vc, hd, s_max * hd, want, hd, G * hd, _i32(ar * (Hq + 2 * Hkv), gpu),
                  _i32(ar * Hkv * s_max, gpu), _i32(klen, gpu), o_start=_i32(ar * Hq, gpu), **kw)
    # rows = the G heads of a group, "heads" = the kv groups: [B * G, Hkv, hd]
    rows = lambda t: t.reshape(B, Hkv, G, hd).transpose(1, 2).reshape(B * G, Hkv, hd)  # noqa: E731
    q_ts = hd + 8
    q_hs = G * q_ts + 16
    q_st = 2 + ar * (-(-Hkv * q_hs // q_ts) + 3)
    _, qs = _place(rows(qkv[:, :Hq * hd]), _flat_index([G] * B, q_st, Hkv, hd, q_ts, q_hs, gpu), q_ts, gpu)
    o_ts = hd + 12
    o_hs = G * o_ts + 8
    o_st = 130 + ar * (-(-Hkv * o_hs // o_ts) + 130)
    out = _Out(_flat_index([G] * B, o_st, Hkv, hd, o_ts, o_hs, gpu), o_ts, gpu)
    keys = torch.cat([kc[b, :, :klen[b]].transpose(0, 1) for b in range(B)])
    vals = torch.cat([vc[b, :, :klen[b]].transpose(0, 1) for b in range(B)])
    k_ts, v_ts = hd + 8, hd + 24
    k_hs, k_st = _cache_layout(B, Hkv, s_max, k_ts)
    v_hs = s_max * v_ts + 40
    assert Hkv * v_hs <= (k_st[1] - k_st[0]) * v_ts
    _, ks = _place(keys, _flat_index(klen, k_st, Hkv, hd, k_ts, k_hs, gpu), k_ts, gpu)
    _, vs = _place(vals, _flat_index(klen, k_st, Hkv, hd, v_ts, v_hs, gpu), v_ts, gpu)
    ops.attention(qs, q_ts, q_hs, ks, k_ts, k_hs, vs, v_ts, v_hs, out.ptr, o_ts, o_hs, _i32(q_st, gpu), _i32(k_st, gpu), _i32(klen, gpu),
                  o_start=_i32(o_st, gpu), **kw)
    torch.cuda.synchronize()
    out.check(rows(want), tag)


@pytest.mark.parametrize("kv_dtype", ["bf16", "fp8"])
@pytest.mark.parametrize("nbuf1", [0, 1 << 30], ids=["one-v-buffer", "two-v-buffers"])
def test_fused_decode_attention_guard_and_strides(gpu, nbuf1, kv_dtype):
    """owc_decode_attention: qkv rows inside a NaN-padded buffer (ld > (n_q + 2 n_kv) * 128), `out` inside canaries with
    ldo > n_q * 128, and every cache row the step may not read - the rows from the write index on, the unused slots - poisoned (bf16
    NaN; fp8: the e4m3fn NaN code and a NaN scale).  The step must overwrite the row at the write index before it reads it."""
    from lmms_owc_amd import _lib, ops

    lib = _lib.load()
    Hq, Hkv, hd, s_max = 12, 2, 128, 264
    klen = np.asarray(DECODE_KLEN)
    B = len(klen)
    tag = f"owc_decode_attention {kv_dtype} decode_attn_nbuf1={nbuf1}"
    r = np.random.default_rng(5)
    slot = r.permutation(B + 2)[:B]
    pos = r.integers(0, 2000, B)
    qkv = bf16_randn((B, (Hq + 2 * Hkv) * hd), 431, 1.0, gpu)
    kc0 = bf16_randn((B + 2, Hkv, s_max, hd), 432, 1.0, gpu)
    vc0 = bf16_randn((B + 2, Hkv, s_max, hd), 433, 1.0, gpu)
    cos, sin = ops.rope_table(2048, 64, 128, 1e6, True, gpu)
    live = torch.zeros((B + 2, Hkv, s_max), dtype=torch.bool, device=gpu)     # rows the step may read: [0, k_len - 1) of its slot
    for b in range(B):
        live[slot[b], :, :klen[b] - 1] = True
    if kv_dtype == "fp8":
        kq, ksc = ops.quantize_rows_fp8(kc0.reshape(-1, hd))
        vq, vsc = ops.quantize_rows_fp8(vc0.reshape(-1, hd))
        caches = [kq.reshape(kc0.shape), vq.reshape(vc0.shape), ksc.reshape(live.shape), vsc.reshape(live.shape)]
        caches[0][~live], caches[1][~live] = POISON[1], POISON[1]
        caches[2][~live], caches[3][~live] = float("nan"), float("nan")
    else:
        caches = [kc0, vc0]
        caches[0][~live], caches[1][~live] = float("nan"), float("nan")

    def run(x, out, cs):
        extra = dict(kv_dtype="fp8", k_scale=cs[2], v_scale=cs[3]) if kv_dtype == "fp8" else {}
        return ops.decode_attention(x, _i32(pos, gpu), cos, sin, cs[0], cs[1], _i32(slot, gpu), _i32(klen - 1, gpu), _i32(klen, gpu), Hq, Hkv, s_max,
                                    hd ** -0.5, out, **extra)

    _, xi = embed(qkv, POISON[2], after=(8, 256 + 40))
    ob, oi = guarded((B, Hq * hd), BF16, gpu, CANARY[2], after=(256, 256 + 72))
    assert oi.stride(0) > Hq * hd and xi.stride(0) > qkv.shape[1] and oi.stride(0) != xi.stride(0)
    try:
        assert lib.owc_tuning_set(b"decode_attn_nbuf1", nbuf1) == 0
        ca, cb = [c.clone() for c in caches], [c.clone() for c in caches]
        want = run(qkv, None, ca)
        run(xi, oi, cb)
        torch.cuda.synchronize()
    finally:
        lib.owc_tuning_set(b"decode_attn_nbuf1", -1)
    assert_guard_intact(ob, oi, tag)
    assert_same_bits(oi, want, tag)
    assert not bool(torch.isnan(oi).any()), f"{tag}: NaN in the output (a poisoned cache row or qkv padding was read)"
    for x, y in zip(ca, cb):       # the two launches leave the same caches
        assert_same_bits(x.reshape(-1, x.shape[-1]), y.reshape(-1, y.shape[-1]), tag + " (caches)")
