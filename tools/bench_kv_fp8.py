"""A/B of the fused decode attention (ops.decode_attention): bf16 KV cache against fp8 (e4m3fn) KV cache, same process, interleaved.

    python tools/bench_kv_fp8.py            # every shape + the end-to-end leg, each in a child process under its own time limit;
                                            # the report goes to profiles/kv_fp8_decode_attention_ab.txt
    python tools/bench_kv_fp8.py --shape 7b_2048x302     # one leg, printed

Per shape: HIP events around groups of launches, `--reps` (>= 20) alternating bf16 / fp8 groups after a warm-up of both; reported
per launch: median, min, max and the spread (max - min) / median of each side, the ratio of the medians, and the bytes a launch
must move (K + V rows, scales included) over the median = achieved GB/s.  Every cache is far larger than the 256 MB Infinity
Cache, so a launch streams it from HBM.  The outputs of the two sides are compared first (same inputs: they differ by the
quantisation only).  `e2e`: one 7B decode step at 2048 rows x ~300 keys, the engine with a bf16 cache against the engine with an fp8
cache on the same synthetic weights - (time of a 17-token generation - time of a 1-token generation) / 16.
"""
import argparse
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

SHAPES = {   # name: (rows, keys, q heads, kv heads)
    "7b_2048x302": (2048, 302, 28, 4),
    "7b_512x540": (512, 540, 28, 4),
    "yi34b_64x2400": (64, 2400, 56, 8),
}
LIMIT_S = {"7b_2048x302": 240, "7b_512x540": 240, "yi34b_64x2400": 240, "e2e": 900}


def shape_leg(name: str, reps: int, group: int) -> None:
    import numpy as np
    import torch

    from lmms_owc_amd import ops

    B, L, Hq, Hkv = SHAPES[name]
    dev = torch.device("cuda:0")
    s_max = (L + 15) // 16 * 16
    g = torch.Generator(device=dev).manual_seed(0)
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
    qkv = torch.randn((B, (Hq + 2 * Hkv) * 128), generator=g, device=dev).to(torch.bfloat16)
    kc = torch.randn((B, Hkv, s_max, 128), generator=g, device=dev).to(torch.bfloat16)
    vc = torch.randn((B, Hkv, s_max, 128), generator=g, device=dev).to(torch.bfloat16)
    k8, ks = ops.quantize_rows_fp8(kc.view(-1, 128))
    v8, vs = ops.quantize_rows_fp8(vc.view(-1, 128))
    cos, sin = ops.rope_table(4096, 64, 128, 1e6, True, dev)
    r = np.random.default_rng(0)
    pos, slot = i32(r.integers(L, 4000, B)), i32(r.permutation(B))
    widx, klen = i32(np.full(B, L - 1)), i32(np.full(B, L))
    out = [torch.empty((B, Hq * 128), dtype=torch.bfloat16, device=dev) for _ in range(2)]

    def bf16():
        ops.decode_attention(qkv, pos, cos, sin, kc, vc, slot, widx, klen, Hq, Hkv, s_max, 128 ** -0.5, out=out[0])

    def fp8():
        ops.decode_attention(qkv, pos, cos, sin, k8, v8, slot, widx, klen, Hq, Hkv, s_max, 128 ** -0.5, out=out[1], kv_dtype="fp8",
                             k_scale=ks, v_scale=vs)

    for _ in range(5):
        bf16()
        fp8()
    torch.cuda.synchronize()
    a, b = out[0].float(), out[1].float()
    print(f"{name}: {B} rows x {L} keys, {Hq} q heads / {Hkv} kv heads; outputs: max |fp8 - bf16| = {(a - b).abs().max().item():.4f} "
          f"of max |bf16| = {a.abs().max().item():.4f}")
    times = {"bf16": [], "fp8": []}
    for _ in range(reps):
        for tag, fn in (("bf16", bf16), ("fp8", fp8)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(group):
                fn()
            e1.record()
            e1.synchronize()
            times[tag].append(e0.elapsed_time(e1) * 1000.0 / group)
    rows = B * Hkv * L
    moved = {"bf16": rows * 2 * 256, "fp8": rows * 2 * 132}
    med = {}
    for tag in ("bf16", "fp8"):
        t = times[tag]
        med[tag] = statistics.median(t)
        print(f"  {tag:5s} cache: median {med[tag]:8.1f} us  min {min(t):8.1f}  max {max(t):8.1f}  spread {(max(t) - min(t)) / med[tag] * 100:5.1f} %  "
              f"({reps} groups of {group} launches, alternating)  {moved[tag] / 1e6:7.1f} MB per launch = {moved[tag] / med[tag] / 1e3:6.0f} GB/s")
    print(f"  fp8 / bf16 = {med['fp8'] / med['bf16']:.3f}  (bytes: {132 / 256:.3f})")


def e2e_leg(reps: int) -> None:
    import numpy as np
    import torch

    from lmms_owc_amd.engine.qwen2vl import DIMS, Qwen2VLDims, Qwen2VLEngine, Qwen2VLWeights

    dev = torch.device("cuda:0")
    r = np.random.default_rng(0)
    prompts = [r.integers(1, 150000, 286).astype(np.int64) for _ in range(2048)]
    none = [[] for _ in prompts]
    eng = {kv: Qwen2VLEngine(Qwen2VLWeights.random(Qwen2VLDims(**{**DIMS["qwen2-vl-7b"].__dict__, "kv_dtype": kv}), dev, seed=1))
           for kv in ("bf16", "fp8")}

    def timed(e, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e.generate(prompts, None, none, n)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    for e in eng.values():
        timed(e, 2)
    step = {"bf16": [], "fp8": []}
    for _ in range(reps):
        for kv, e in eng.items():
            t1, t17 = timed(e, 1), timed(e, 17)
            step[kv].append((t17 - t1) / 16 * 1e3)
    print(f"e2e: Qwen2-VL-7B (synthetic weights), 2048 rows x 286-302 keys, one decode step = (17-token - 1-token generation) / 16, {reps} alternating repetitions")
    for kv in ("bf16", "fp8"):
        t = step[kv]
        print(f"  {kv:5s} cache: median {statistics.median(t):7.2f} ms per step  min {min(t):7.2f}  max {max(t):7.2f}   KV cache {eng[kv].kv_bytes(2048, 304) / 1e9:.2f} GB")
    print(f"  fp8 / bf16 = {statistics.median(step['fp8']) / statistics.median(step['bf16']):.3f}")


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=list(SHAPES) + ["e2e"])
    ap.add_argument("--reps", type=int, default=24)
    ap.add_argument("--group", type=int, default=10)
    ap.add_argument("--e2e-reps", type=int, default=3)
    ap.add_argument("--no-e2e", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "kv_fp8_decode_attention_ab.txt"))
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20")
    if a.shape == "e2e":
        e2e_leg(a.e2e_reps)
        return 0
    if a.shape:
        shape_leg(a.shape, a.reps, a.group)
        return 0
    # every leg in a fresh child under its own time limit; the first failure ends the run (nothing more is started on the GPU)
    report = [f"# tools/bench_kv_fp8.py --reps {a.reps} --group {a.group}: fused decode attention, bf16 KV cache vs fp8 (e4m3fn) KV cache"]
    rc = 0
    for leg in list(SHAPES) + ([] if a.no_e2e else ["e2e"]):
        cmd = ["timeout", "-k", "10", str(LIMIT_S[leg]), sys.executable, __file__, "--shape", leg, "--reps", str(a.reps), "--group", str(a.group),
               "--e2e-reps", str(a.e2e_reps)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        text = p.stdout.strip()
        print(text, flush=True)
        report.append(text)
        if p.returncode != 0:
            print(p.stderr[-2000:], file=sys.stderr)
            report.append(f"{leg}: FAILED with exit status {p.returncode}")
            rc = p.returncode
            break
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(report) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
