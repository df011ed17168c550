"""What the straggler hand-over is worth under the checkpoint's repetition penalty: `bench.eos_terminated_leg` (max_new_tokens 256,
the default seeded ragged answer lengths, a task of three passes) on the 7B engine with random weights, with
`engine.repetition_penalty` at 1.0 and at 1.05 alternating, `--repeats` times each.  Appends one block to `--out`: images/s of
"compacted, one pass" and of "passes_with_straggler_hand_over" (median, min .. max) and the handed-over counts per pass.

usage: python tools/bench_handover_penalty.py [--repo DIR] [--label NAME] [--out FILE] [--batch 2048] [--repeats 3] [--model qwen2-vl-7b]
`--repo DIR` measures the package of ANOTHER source tree (e.g. an export of the parent commit with the built library beside it) with
this same script, so both figures of a comparison come from one session on one GPU."""
import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--repo", default=str(Path(__file__).resolve().parent.parent))
ap.add_argument("--label", default="this tree")
ap.add_argument("--out", default="profiles/handover_penalty.txt")
ap.add_argument("--batch", type=int, default=2048)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--model", default="qwen2-vl-7b")
ap.add_argument("--penalties", default="1.0,1.05")
args = ap.parse_args()
sys.path.insert(0, args.repo)
import bench  # noqa: E402
from lmms_owc_amd import ops  # noqa: E402
from lmms_owc_amd.engine.qwen2vl import DIMS, Qwen2VLEngine, Qwen2VLWeights  # noqa: E402
from lmms_owc_amd.models import imageproc  # noqa: E402

dev = torch.device("cuda:0")
d = DIMS[args.model]
B = args.batch
eng = Qwen2VLEngine(Qwen2VLWeights.random(d, dev, seed=1234))
gen = torch.Generator(device=dev).manual_seed(1234)
pix = torch.empty((B * 1024, 1176), device=dev, dtype=torch.bfloat16)      # the bench's input: 448 x 448 uniform-noise images
for i0 in range(0, B, 256):
    n_i = min(256, B - i0)
    u8 = torch.randint(0, 256, (n_i, 3, 448, 448), generator=gen, device=dev, dtype=torch.uint8)
    ops.patchify_u8(u8, imageproc.OPENAI_CLIP_MEAN, imageproc.OPENAI_CLIP_STD, out=pix[i0 * 1024:(i0 + n_i) * 1024])
del u8
prompts = [bench.prompt_ids(d.image_token_id)] * B
grids, flat = [[(1, 32, 32)]] * B, [(1, 32, 32)] * B


def sync():
    torch.cuda.synchronize()
    return time.perf_counter()


n_w = min(B, 256)   # warm-up: code objects, workspace
eng.generate(prompts[:n_w], eng.encode_images(pix[:n_w * 1024], flat[:n_w]), grids[:n_w], 8).cpu()
penalties = [float(p) for p in args.penalties.split(",")]
runs = {p: [] for p in penalties}
for rep in range(args.repeats):
    for p in penalties:
        eng.repetition_penalty = p
        row = bench.eos_terminated_leg(eng, pix, flat, prompts, grids, B, sync, 1.0, 0, caps=(256,), plain_caps=())["by_cap"][0]
        if "skipped" in row:
            raise SystemExit(f"max_new_tokens 256 does not fit at batch {B}: {row['skipped']}")
        runs[p].append(row)
        ho = row.get("passes_with_straggler_hand_over", {})
        print(f"[{args.label}] repeat {rep} penalty {p}: one pass {row['compacted']['images_per_s']:.1f} images/s, three passes "
              f"{ho.get('images_per_s', float('nan')):.1f} images/s, handed over {ho.get('sequences_handed_to_the_next_pass')}", flush=True)


def stat(vals) -> str:
    return f"median {statistics.median(vals):7.1f}  (min {min(vals):7.1f} .. max {max(vals):7.1f}, n = {len(vals)})"


lines = [f"== {args.label}: {args.model}, random weights, {B} images per pass, max_new_tokens 256, "
         f"{runs[penalties[0]][0]['mean_answer_tokens']:.1f} answer tokens on average, {torch.cuda.get_device_name(0)}"]
for p in penalties:
    one = [r["compacted"]["images_per_s"] for r in runs[p]]
    ho = [r["passes_with_straggler_hand_over"] for r in runs[p] if "passes_with_straggler_hand_over" in r]
    lines.append(f"repetition_penalty {p}")
    lines.append(f"  compacted, one pass              images/s  {stat(one)}")
    if ho:
        three = [h["images_per_s"] for h in ho]
        lines.append(f"  passes_with_straggler_hand_over  images/s  {stat(three)}")
        lines.append(f"    relative to one pass: {statistics.median(three) / statistics.median(one):.3f};  sequences handed to the next pass: "
                     f"{[h['sequences_handed_to_the_next_pass'] for h in ho]};  tokens identical to a pass run alone: "
                     f"{all(h['tokens_identical_to_a_pass_run_alone'] for h in ho)}")
out = Path(args.out)
out.parent.mkdir(parents=True, exist_ok=True)
with out.open("a") as f:
    f.write("\n".join(lines) + "\n\n")
print("\n".join(lines))
